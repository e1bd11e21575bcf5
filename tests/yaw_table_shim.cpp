// yaw_table_shim.cpp — hands the node rule of windgym_amd/csrc/wg_yaw_table.h to tests/test_yaw_table.py.  Host C++ only:
//   g++ -std=c++17 -shared -fPIC -I windgym_amd/csrc tests/yaw_table_shim.cpp
#include "wg_yaw_table.h"

// the node of each of n values on the axis a [n_a]
extern "C" void yt_axis(const double* a, int n_a, int wrap, const double* x, int n, int* out) {
    for (int i = 0; i < n; ++i) out[i] = wg_yt_axis(a, n_a, x[i], wrap);
}

// the row of each of n winds (ws, wd, ti); ax: the axes ti, ws, wd back to back
extern "C" void yt_rows(const double* ax, int n_ti, int n_ws, int n_wd, int wrap_wd, const double* wind, int n, int* out) {
    for (int i = 0; i < n; ++i) out[i] = wg_yt_row(ax, n_ti, n_ws, n_wd, wrap_wd, wind[3 * i], wind[3 * i + 1], wind[3 * i + 2]);
}

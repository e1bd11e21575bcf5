// wg_api.hip — host side of libwindgym_hip.so: the C ABI declared in include/windgym_hip.h.
// Owns the device state (allocated once in wg_create; nothing is allocated on the step path) and launches
// the kernels of wg_kernels.hip on the caller's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "wg_plan.h"
#include "wg_steady.h"
#include "wg_policy.h"
#include "wg_lstm.h"
#include "wg_host.h"

// Measurement / test hooks (environment variables that select kernel variants): honoured ONLY with WG_DEBUG_HOOKS=1 — a
// stray WG_FLOW_BLOCK in a user's shell must not silently change the kernel — and announced once on stderr when used.
// (binding.py guards its own hooks, WG_LIB / WG_NOCHECK, the same way; tests/conftest.py sets the switch)
static const char* wg_hook(const char* name) {
    static const bool on = [] { const char* v = getenv("WG_DEBUG_HOOKS"); return v && v[0] == '1' && v[1] == 0; }();
    if (!on) return nullptr;
    const char* v = getenv(name);
    if (v) {
        static std::string seen;
        static std::mutex seen_mu;      // (wg_create may run on several threads at once: one handle per device)
        std::lock_guard<std::mutex> lock(seen_mu);
        const std::string tag = std::string(name) + "=" + v + ";";
        if (seen.find(tag) == std::string::npos) {
            seen += tag;
            fprintf(stderr, "[windgym] WG_DEBUG_HOOKS: %s=%s\n", name, v);
        }
    }
    return v;
}
// Every hook as a value, read once per wg_create (the kernel plan, wg_plan.h, is a function of these values).  The box setters
// read them again: the stencil-record A/B test switches WG_NO_BOX8 between wg_create and wg_set_turbulence_box.
static WgHooks wg_hooks_read() {
    WgHooks k;
    const auto num = [](const char* name) { WgHookInt r; if (const char* v = wg_hook(name)) { r.set = true; r.v = atoi(v); } return r; };
    k.flow_block = num("WG_FLOW_BLOCK"); k.flow_res = num("WG_FLOW_RES"); k.flow_env = num("WG_FLOW_ENV");
    k.env_wpe = num("WG_ENV_WPE"); k.env_split = num("WG_ENV_SPLIT"); k.step_fused = num("WG_STEP_FUSED");
    k.sums = num("WG_SUMS"); k.lds_pad = num("WG_LDS_PAD"); k.lf_cap = num("WG_LF_CAP"); k.pstride_pad = num("WG_PSTRIDE_PAD");
    k.step_graph = num("WG_STEP_GRAPH"); k.share_dev = num("WG_ENV_SHARE_DEV");
    k.first_obs_gl_only = wg_hook("WG_FIRST_OBS_GL_ONLY") != nullptr;
    k.no_box8 = wg_hook("WG_NO_BOX8") != nullptr;
    k.debug = wg_hook("WG_DEBUG") != nullptr;
    if (const char* v = wg_hook("WG_TIMELINE_OUT")) { k.timeline = true; k.timeline_out = v; }
    return k;
}

static thread_local std::string g_err;
// (every translation unit of the library reports through this thread-local message: wg_host.h's wg_fail, wg_mann.hip)
extern "C" int wg_set_last_error_(int code, const char* msg) {
    g_err = msg ? msg : "";
    return code;
}

struct Alloc {
    void* ptr;
    size_t bytes;
};

struct wg_env_s {
    WgPlan plan;                    // what wg_create decided (wg_plan.h); never changed afterwards
    WgHooks hooks;                  // the measurement hooks as wg_create read them
    WgParams p;                     // the kernels' parameter blocks: copies of plan.p / plan.f that follow the setters
    WgPtrs d;
    FlowP fp;
    FlowPtrs fd;
    unsigned long long flow_steps_mark = 0, particles_mark = 0, added_mark = 0;
    double added_per_launch = 0.0;  // window closed by the last wg_kernel_timing
    long n_step_launches = 0;
    void* box4 = nullptr;            // interleaved copy of the caller's turbulence box (owned)
    void* box4c = nullptr;           // block-averaged copy for the particle lookups (owned)
    int* box_ids_dev = nullptr;      // wg_set_box_ids
    void* abox4 = nullptr;           // interleaved isotropic box of the wake-added turbulence (owned)
    void* box8 = nullptr;            // stencil records of the box pool / of the wake-added box (owned; FlowPtrs::box8, k_flow_envb)
    void* abox8 = nullptr;
    double* wind_dev = nullptr;      // per-env wind override (wg_set_wind)
    int device;
    WgDevMem mem;                   // owns every device buffer of the handle, the box copies above included
    std::vector<Alloc> allocs;      // what wg_create allocated, in order (state blob = allocs flagged `state`)
    std::vector<size_t> state_idx;  // indices into allocs that make up the serialisable state
    uint8_t* mask_dev = nullptr;
    uint64_t* seeds_dev = nullptr;
    // timing
    bool timing = false;
    int timing_period = 1, timing_phase = 0;   // record events around every `period`-th step() only
    std::vector<hipEvent_t> ev;     // pairs (start, stop) around flow launches, then glue launches
    std::vector<int> ev_kind;
    size_t ev_used = 0;
    // step() as ONE graph launch: the launches of a step are captured once per distinct set of I/O pointers on an
    // internal stream and replayed on the caller's stream (wg_set_step_graph)
    struct StepGraph {
        const void* key[5];
        hipGraph_t graph;
        hipGraphExec_t exec;
        unsigned long long last_use;
    };
    std::vector<StepGraph> graphs;
    hipStream_t cap_stream = nullptr;
    int graph_mode = 0;
    unsigned long long graph_clock = 0;
    int* unready_dev = nullptr;     // wg_reset: live slots of the masked envs that are not developed yet
    WgParams* p_dev = nullptr;      // device copies of p / d, read by the episode-initialisation path at the head of k_flow
    WgPtrs* d_dev = nullptr;
    float* flat_scratch = nullptr;  // [B][obs_dim]: where wg_rollout_multi's steps put the flat observation nobody asked for
};

static const size_t WG_MAX_STEP_GRAPHS = 32;   // distinct (actions, obs, reward, truncated, final_obs) pointer sets cached
static const size_t WG_MAX_TIMING_EVENTS = 4096;

static void drop_step_graphs(wg_env_s* h) {
    // a cached exec may still be in flight on the caller's stream: destroying it under a running launch is undefined
    if (!h->graphs.empty()) { hipSetDevice(h->device); hipDeviceSynchronize(); }
    for (auto& g : h->graphs) {
        hipGraphExecDestroy(g.exec);
        hipGraphDestroy(g.graph);
    }
    h->graphs.clear();
}

// the device copies of the parameter blocks follow every host-side change (setters are rare, synchronous calls)
static int sync_dev_params(wg_env_s* h) {
    hipError_t e = hipMemcpy(h->p_dev, &h->p, sizeof(WgParams), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->d_dev, &h->d, sizeof(WgPtrs), hipMemcpyHostToDevice);
    if (e != hipSuccess) return wg_fail(WG_ERR_HIP, std::string("hipMemcpy(params): ") + hipGetErrorString(e));
    return 0;
}

template <typename T>
static int dev_alloc(wg_env_s* h, T** out, size_t n, bool state, bool zero = true) {
    if (int rc = h->mem.alloc("wg_create", out, n, zero)) return rc;
    h->allocs.push_back({*out, sizeof(T) * (n ? n : 1)});
    if (state) h->state_idx.push_back(h->allocs.size() - 1);
    return 0;
}
template <typename T, typename S>
static int dev_upload(wg_env_s* h, const T** out, const S* src, size_t n) {
    std::vector<T> tmp(n ? n : 1);
    for (size_t i = 0; i < n; ++i) tmp[i] = (T)src[i];
    T* p = nullptr;
    int rc = dev_alloc(h, &p, n, false, false);
    if (rc) return rc;
    WG_HIPCHK(hipMemcpy(p, tmp.data(), sizeof(T) * (n ? n : 1), hipMemcpyHostToDevice));
    *out = p;
    return 0;
}

extern "C" const char* wg_last_error(void) { return g_err.c_str(); }
extern "C" int wg_abi_version(void) { return WG_ABI_VERSION; }

// ---- wg_create: validate -> hooks -> plan (wg_plan.h) -> allocate -> upload -> kernel pointer blocks -> initialise -------------
// the half-built handle has one owner: every early return destroys it
struct HandleGuard {
    void operator()(wg_env_s* h) const { wg_destroy(h); }
};

static int create_alloc(wg_env_s* h) {
    const WgParams& p = h->p;
    WgPtrs& d = h->d;
    const size_t n_slots = (size_t)p.B * 2 * p.F, n_ctx = (size_t)p.B * 2, pstride = (size_t)h->fp.pstride;
    int rc = 0;
#define A(field, n, st) if (!rc) rc = dev_alloc(h, &d.field, (n), (st))
    A(py, n_slots * pstride, true);     // (rec_a / rec_b: create_alloc_record, after the tables — the state blob keeps its order)
    if (p.turb_mode != WG_TURB_NONE) {
        A(pz, n_slots * pstride, true); A(vlp, n_slots * pstride, true); A(wlp, n_slots * pstride, true);
    }
    A(yaw, n_slots * p.N, true); A(u, n_slots * p.N, true); A(v, n_slots * p.N, true); A(w, n_slots * p.N, true);
    A(ti_loc, n_slots * p.N, true); A(power, n_slots * p.N, true); A(ct, n_slots * p.N, true);
    A(bnd, n_slots * p.N * 4, true);
    A(slot, n_slots, true); A(ctx, n_ctx, true); A(env, (size_t)p.B, true);
    A(xr, n_ctx * p.N, true); A(yr, n_ctx * p.N, true); A(jneed, n_ctx * p.N, true);
    A(roff, n_ctx * (p.N + 1), true); A(qown, n_ctx * (size_t)(p.NP / 4), true);
    A(ring, n_ctx * p.ring_stride, true); A(fring, n_ctx * p.fring_stride, true);
    A(cur_ws, n_ctx * p.N, true); A(cur_wd, n_ctx * p.N, true);
    A(pend_farm, n_ctx * p.power_avg, true); A(pend_base, n_ctx * p.power_avg, true);
    A(farm_pow, (size_t)p.B * p.power_avg, true); A(base_pow, (size_t)p.B * p.power_avg, true);
    A(old_yaw, (size_t)p.B * p.N, true);
    A(step_farm_pow, (size_t)p.B, true); A(step_base_pow, (size_t)p.B, true);
    A(last_pow_agent, (size_t)p.B, true); A(last_pow_base, (size_t)p.B, true);
    A(metrics, (size_t)p.B * WG_N_METRICS, true);
    if (h->plan.first_obs) { A(next_obs, n_ctx * (size_t)p.obs_dim, false); A(next_obs_ok, n_ctx, false); }
    if (p.sums_mode) A(wsum, n_ctx * WG_N_SUMS * (size_t)(p.N + 1), true);
    A(status, 1, true);
#undef A
    if (!rc) rc = dev_alloc(h, &h->mask_dev, (size_t)p.B, false);
    if (!rc) rc = dev_alloc(h, &h->seeds_dev, (size_t)p.B, false);
    if (!rc) rc = dev_alloc(h, &h->unready_dev, 1, false);
    if (!rc) rc = dev_alloc(h, &h->p_dev, 1, false);
    if (!rc) rc = dev_alloc(h, &h->d_dev, 1, false);
    return rc;
}

// packed emission record: two arrays, or one interleaved array (FlowP::rec_il)
static int create_alloc_record(wg_env_s* h) {
    const size_t n = (size_t)h->p.B * 2 * h->p.F * (size_t)h->fp.pstride;
    if (h->fp.rec_il) {
        if (int rc = dev_alloc(h, &h->d.rec_a, 2 * n, true)) return rc;
        h->d.rec_b = h->d.rec_a + 1;
        return 0;
    }
    if (int rc = dev_alloc(h, &h->d.rec_a, n, true)) return rc;
    return dev_alloc(h, &h->d.rec_b, n, true);
}

static int create_upload(wg_env_s* h, const wg_config* c) {
    const WgParams& p = h->p;
    WgPtrs& d = h->d;
    int rc = dev_upload<double>(h, &d.x_pos, c->x_pos, p.N);
    if (!rc) rc = dev_upload<double>(h, &d.y_pos, c->y_pos, p.N);
    if (!rc && c->yaw_defined) rc = dev_upload<double>(h, &d.yaw_defined, c->yaw_defined, p.N);
    if (!rc) {
        // PCG64 k draws ahead, k = 0 .. max(N, 3): the LCG step s -> M s + inc composed k times is s -> A_k s + G_k inc with A_k = M^k,
        // G_k = 1 + M + ... + M^(k-1) (mod 2^128) — the N yaw draws of an episode set-up are then one draw per lane
        const int kmax = std::max(p.N, 3);             // (k = 3: the state after the three wind draws)
        std::vector<uint64_t> jump((size_t)(kmax + 1) * 4);
        wg_u128 A = 1, G = 0;
        for (int k = 0; k <= kmax; ++k) {
            jump[4 * (size_t)k] = (uint64_t)A; jump[4 * (size_t)k + 1] = (uint64_t)(A >> 64);
            jump[4 * (size_t)k + 2] = (uint64_t)G; jump[4 * (size_t)k + 3] = (uint64_t)(G >> 64);
            A = A * WG_PCG_MULT; G = G * WG_PCG_MULT + 1;
        }
        rc = dev_upload<uint64_t>(h, &d.pcg_jump, jump.data(), jump.size());
    }
    if (!rc) rc = dev_upload<float>(h, &d.rotor_dy, c->rotor_dy, p.S);
    if (!rc) rc = dev_upload<float>(h, &d.rotor_dz, c->rotor_dz, p.S);
    if (!rc) rc = dev_upload<float>(h, &d.tab_ws, c->tab_ws, p.n_tab);
    if (!rc) rc = dev_upload<float>(h, &d.tab_power, c->tab_power, p.n_tab);
    if (!rc) rc = dev_upload<float>(h, &d.tab_ct, c->tab_ct, p.n_tab);
    if (!rc) rc = dev_upload<double>(h, &d.tab_ws_d, c->tab_ws, p.n_tab);
    if (!rc) rc = dev_upload<double>(h, &d.tab_power_d, c->tab_power, p.n_tab);
    if (rc) return rc;
    // the flow kernels' turbine table, on the uniform grid of the plan
    std::vector<float> pu, cu;
    double x0 = 0, dx = 0;
    wg_uniform_table(c, &pu, &cu, &x0, &dx);
    rc = dev_upload<float>(h, &h->fd.tab_power, pu.data(), pu.size());
    if (!rc) rc = dev_upload<float>(h, &h->fd.tab_ct, cu.data(), cu.size());
    return rc;
}

// k_flow's pointer block: the arrays of WgPtrs it works on (tab_power / tab_ct: create_upload)
static void create_flow_ptrs(wg_env_s* h) {
    const WgPtrs& d = h->d;
    FlowPtrs& g = h->fd;
    g.py = d.py; g.rec_a = d.rec_a; g.rec_b = d.rec_b;
    g.pz = d.pz; g.vlp = d.vlp; g.wlp = d.wlp;
    g.bnd = d.bnd;
    g.yaw = d.yaw; g.u = d.u; g.v = d.v; g.w = d.w; g.ti_loc = d.ti_loc; g.power = d.power; g.ct = d.ct;
    g.slot = d.slot; g.ctx = d.ctx; g.env = d.env; g.xr = d.xr; g.yr = d.yr; g.jneed = d.jneed;
    g.ring = d.ring; g.fring = d.fring; g.cur_ws = d.cur_ws; g.cur_wd = d.cur_wd;
    g.pend_farm = d.pend_farm; g.pend_base = d.pend_base; g.old_yaw = d.old_yaw;
    g.step_farm_pow = d.step_farm_pow; g.step_base_pow = d.step_base_pow;
    g.rotor_dy = d.rotor_dy; g.rotor_dz = d.rotor_dz;
    g.gp = h->p_dev; g.gd = h->d_dev; g.env_rw = d.env;
    g.roff = d.roff; g.qown = d.qown; g.status = d.status;
}

// fp.envw / fp.env_fused from the plan and the boxes set at the moment
static void apply_step_path(wg_env_s* h) {
    wg_plan_step_path(h->plan, h->fp.box_cells, (long long)h->fp.anx * h->fp.any * h->fp.anz, &h->fp.envw, &h->fp.env_fused);
}

extern "C" int wg_create(const wg_config* c, int device, wg_handle* out) {
    if (!c || !out) return wg_fail(WG_ERR_INVALID, "null argument");
    std::string err;
    if (int rc = wg_validate_config(c, &err)) return wg_fail(rc, err);
    WG_HIPCHK(hipSetDevice(device));
    int lds_limit = 65536;
    {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && v > 0)
            lds_limit = std::min(v, 65536);      // (no kernel opts in to more than the default 64 KB of dynamic LDS)
    }
    std::unique_ptr<wg_env_s, HandleGuard> owner(new wg_env_s());      // (value-initialised: every pointer of d / fd starts null)
    wg_env_s* h = owner.get();
    h->mem.device = h->device = device;
    h->hooks = wg_hooks_read();
    if (int rc = wg_plan_create(c, h->hooks, lds_limit, &h->plan, &err)) return wg_fail(rc, err);
    h->p = h->plan.p;
    h->fp = h->plan.f;
    apply_step_path(h);

    if (int rc = create_alloc(h)) return rc;
    if (int rc = create_upload(h, c)) return rc;
    if (int rc = create_alloc_record(h)) return rc;
    create_flow_ptrs(h);
    if (h->hooks.timeline) {      // -DWG_TIMELINE builds: phase stamps of the last launch (dumped by wg_destroy)
        long long* dbgp = nullptr;
        if (!dev_alloc(h, &dbgp, (size_t)h->p.B * 2 * h->p.F * 16, false)) h->fd.dbg = dbgp;
    }
    wg_launch_create(&h->p, &h->d, nullptr);
    if (sync_dev_params(h)) return WG_ERR_HIP;
    {
        hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking);
        if (e != hipSuccess) return wg_fail(WG_ERR_HIP, std::string("wg_create: ") + hipGetErrorString(e));
    }
    if (h->hooks.step_graph.set) h->graph_mode = h->hooks.step_graph.v != 0;
    if (h->hooks.debug) {
        const FlowP& f = h->fp;
        fprintf(stderr, "[windgym] k_flow variant: %s%s, %d threads, LDS %d B per workgroup, slot stride %d floats\n",
                f.envw ? (f.turb_mode == WG_TURB_NONE ? "compact rings / pair-major, one wave per env (k_flow_env)" : "compact rings / sample-major, one wave per env (k_flow_envb)")
                       : (f.res ? "compact rings / pair-major" : "uniform rings / sample-major"),
                f.envw && f.env_split ? " + a pass wave for the running episode's context" : "",
                f.block, f.envw ? f.env_lds : f.lds_bytes, f.pstride);
        fprintf(stderr, "[windgym] plan: res %d block %d gl %d rec_il %d target_chunk %d lf_cap %d lds_bytes %d | envw %d env_wpe %d env_split %d env_fused %d "
                        "env_share %d env_lds %d env_off_tab %d | sums_mode %d first_obs %d reset_launches %d\n",
                f.res, f.block, f.gl, f.rec_il, f.target_chunk, f.lf_cap, f.lds_bytes, f.envw, f.env_wpe, f.env_split, f.env_fused, f.env_share,
                f.env_lds, f.env_off_tab, h->p.sums_mode, h->plan.first_obs, h->plan.reset_launches);
    }
    *out = owner.release();
    return 0;
}

extern "C" int wg_destroy(wg_handle h) {
    if (!h) return 0;
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    if (h->fd.dbg && h->hooks.timeline) {      // -DWG_TIMELINE builds: dump the phase stamps of the last launch
        const size_t n = (size_t)h->p.B * 2 * h->p.F * 16;
        std::vector<long long> host(n);
        if (hipMemcpy(host.data(), h->fd.dbg, n * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess) {
            if (FILE* f = fopen(h->hooks.timeline_out.c_str(), "wb")) { fwrite(host.data(), sizeof(long long), n, f); fclose(f); }
        }
    }
    drop_step_graphs(h);
    if (h->cap_stream) hipStreamDestroy(h->cap_stream);
    for (auto& e : h->ev) hipEventDestroy(e);
    h->mem.release();
    delete h;
    return 0;
}

extern "C" int wg_obs_dim(wg_handle h, int* obs_dim, int* obs_dim_multi) {
    if (!h) return wg_fail(WG_ERR_INVALID, "null handle");
    if (obs_dim) *obs_dim = h->p.obs_dim;
    if (obs_dim_multi) *obs_dim_multi = h->p.obs_dim_multi;
    return 0;
}
extern "C" int wg_hist_max(wg_handle h, int* hist_max) {
    if (!h || !hist_max) return wg_fail(WG_ERR_INVALID, "null argument");
    *hist_max = h->p.hist_max;
    return 0;
}

// Stencil records of a box pool (FlowPtrs::box8 / abox8) for handles that run k_flow_envb: 8 x the interleaved copy.  Built only
// while the whole pool's records stay below a quarter of the device memory and a box below 2^28 cells (32-bit record offsets);
// otherwise the kernel keeps reading the brick-ordered box (same cells, same weights: the results are identical either way).
// a box copy that a setter replaces: forgotten first (a failure must not leave the handle pointing at freed memory), then freed
static int drop_box(wg_env_s* h, const char* who, void** box) {
    void* const q = *box;
    *box = nullptr;
    return h->mem.free(who, q);
}

static int build_stencil_records(wg_env_s* h, void** owned, const float4** kernel_ptr, const void* box4, int n_boxes, int nx, int ny, int nz) {
    *kernel_ptr = nullptr;
    if (!(h->fp.envw && h->fp.turb_mode != WG_TURB_NONE)) return 0;      // (no k_flow_envb on this handle: nothing reads them)
    const auto skip = [h](const char* why) {
        if (h->hooks.debug) fprintf(stderr, "[windgym] stencil records not built (%s): k_flow_envb reads the brick-ordered box\n", why);
        return 0;
    };
    if (wg_hooks_read().no_box8) return skip("WG_NO_BOX8");
    const size_t n_cells = (size_t)nx * ny * nz, bytes = n_cells * 128 * (size_t)n_boxes;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return skip("hipMemGetInfo failed");
    if (n_cells >= ((size_t)1 << 28)) return skip("a box of 2^28 cells or more");
    if (bytes > total_b / 4 || bytes > free_b / 2) return skip("the pool's records exceed a quarter of the device memory or half of what is free");
    if (h->mem.alloc_bytes("stencil records", owned, bytes, false)) { (void)hipGetLastError(); return skip("hipMalloc failed"); }
    for (int k = 0; k < n_boxes; ++k)
        wg_launch_box_stencil((const char*)box4 + (size_t)k * n_cells * 16, (char*)*owned + (size_t)k * n_cells * 128, nx, ny, nz, nullptr);
    WG_HIPCHK(hipDeviceSynchronize());
    *kernel_ptr = (const float4*)*owned;
    return 0;
}

extern "C" int wg_set_turbulence_boxes(wg_handle h, const float* const* boxes_dev, int n_boxes, int nx, int ny, int nz,
                                       double dx, double dy, double dz) {
    if (!h) return wg_fail(WG_ERR_INVALID, "null handle");
    if (!boxes_dev || n_boxes < 1 || n_boxes > 64 || nx < 2 || ny < 2 || nz < 2 || !(dx > 0) || !(dy > 0) || !(dz > 0))
        return wg_fail(WG_ERR_INVALID, "turbulence box: null pointer, bad pool size (1..64) or bad dimensions");
    for (int k = 0; k < n_boxes; ++k)
        if (!boxes_dev[k]) return wg_fail(WG_ERR_INVALID, "turbulence box: null pointer in the pool");
    WG_HIPCHK(hipSetDevice(h->device));
    WG_HIPCHK(hipDeviceSynchronize());
    drop_step_graphs(h);           // the kernel arguments captured in them are about to change
    // the kernel-side pointers are cleared first: a failure below must not leave them dangling
    h->d.box = nullptr; h->fd.box4 = nullptr; h->fd.box4c = nullptr; h->fd.box8 = nullptr; h->fp.coarse = 0;
    for (void** box : {&h->box8, &h->box4, &h->box4c})
        if (int rc = drop_box(h, "wg_set_turbulence_boxes", box)) return rc;
    const size_t n_cells = (size_t)nx * ny * nz;
    if (int rc = h->mem.alloc_bytes("wg_set_turbulence_boxes", &h->box4, n_cells * 16 * (size_t)n_boxes, false)) return rc;
    for (int k = 0; k < n_boxes; ++k)
        wg_launch_box_repack(boxes_dev[k], (char*)h->box4 + (size_t)k * n_cells * 16, nx, ny, nz, nullptr);
    WG_HIPCHK(hipDeviceSynchronize());
    h->d.box = boxes_dev[0];
    h->p.n_boxes = n_boxes;
    h->p.bnx = nx; h->p.bny = ny; h->p.bnz = nz; h->p.bdx = dx; h->p.bdy = dy; h->p.bdz = dz;
    h->fd.box4 = (const float4*)h->box4;
    h->fp.bnx = nx; h->fp.bny = ny; h->fp.bnz = nz; h->fp.box_cells = (long long)n_cells;
    apply_step_path(h);
    h->fp.box_pow2 = ((nx & (nx - 1)) == 0) && ((ny & (ny - 1)) == 0) && ((nz & (nz - 1)) == 0);
    h->fp.coarse = (nx % 4 == 0 && ny % 4 == 0 && nz % 4 == 0 && nx >= 8 && ny >= 8 && nz >= 8);
    h->fd.box4c = nullptr;
    if (h->fp.coarse) {
        const int cx = nx / 4, cy = ny / 4, cz = nz / 4;
        const size_t c_cells = (size_t)cx * cy * cz;
        if (int rc = h->mem.alloc_bytes("wg_set_turbulence_boxes", &h->box4c, c_cells * 16 * (size_t)n_boxes, false)) return rc;
        for (int k = 0; k < n_boxes; ++k)
            wg_launch_box_coarsen((const char*)h->box4 + (size_t)k * n_cells * 16, (char*)h->box4c + (size_t)k * c_cells * 16,
                                  nx, ny, nz, nullptr);
        WG_HIPCHK(hipDeviceSynchronize());
        h->fp.cnx = cx; h->fp.cny = cy; h->fp.cnz = cz; h->fp.cbox_cells = (long long)c_cells;
        h->fp.cbox_pow2 = ((cx & (cx - 1)) == 0) && ((cy & (cy - 1)) == 0) && ((cz & (cz - 1)) == 0);
        h->fd.box4c = (const float4*)h->box4c;
    }
    h->fp.inv_bdx = 1.0 / dx; h->fp.inv_bdy = 1.0 / dy; h->fp.inv_bdz = 1.0 / dz;
    h->fp.inv_bn[0] = 1.0 / nx; h->fp.inv_bn[1] = 1.0 / ny; h->fp.inv_bn[2] = 1.0 / nz;
    if (int rc = build_stencil_records(h, &h->box8, &h->fd.box8, h->box4, n_boxes, nx, ny, nz)) return rc;
    return sync_dev_params(h);
}

extern "C" int wg_set_added_turbulence_box(wg_handle h, const float* box_dev, int nx, int ny, int nz, double dx,
                                           double dy, double dz) {
    if (!h || !box_dev || nx < 2 || ny < 2 || nz < 2 || !(dx > 0) || !(dy > 0) || !(dz > 0))
        return wg_fail(WG_ERR_INVALID, "added-turbulence box: null pointer or bad dimensions");
    WG_HIPCHK(hipSetDevice(h->device));
    WG_HIPCHK(hipDeviceSynchronize());
    drop_step_graphs(h);
    h->fd.abox4 = nullptr; h->fd.abox8 = nullptr;
    for (void** box : {&h->abox8, &h->abox4})
        if (int rc = drop_box(h, "wg_set_added_turbulence_box", box)) return rc;
    const size_t n_cells = (size_t)nx * ny * nz;
    if (int rc = h->mem.alloc_bytes("wg_set_added_turbulence_box", &h->abox4, n_cells * 16, false)) return rc;
    wg_launch_box_repack(box_dev, h->abox4, nx, ny, nz, nullptr);
    WG_HIPCHK(hipDeviceSynchronize());
    h->fd.abox4 = (const float4*)h->abox4;
    h->fp.anx = nx; h->fp.any = ny; h->fp.anz = nz;
    apply_step_path(h);
    h->fp.abox_pow2 = ((nx & (nx - 1)) == 0) && ((ny & (ny - 1)) == 0) && ((nz & (nz - 1)) == 0);
    h->fp.inv_adx = 1.0 / dx; h->fp.inv_ady = 1.0 / dy; h->fp.inv_adz = 1.0 / dz;
    h->fp.inv_an[0] = 1.0 / nx; h->fp.inv_an[1] = 1.0 / ny; h->fp.inv_an[2] = 1.0 / nz;
    if (int rc = build_stencil_records(h, &h->abox8, &h->fd.abox8, h->abox4, 1, nx, ny, nz)) return rc;
    return 0;
}

extern "C" int wg_set_deficit_table(wg_handle h, const float* table_dev, int n_ct, double ct0, double ct1, int n_ti, double ti0,
                                    double ti1, int n_x, double x_max_D, int n_r, double r_max_R) {
    if (!h || !table_dev || n_ct < 2 || n_ti < 2 || n_x < 2 || n_r < 2 || !(ct1 > ct0) || !(ti0 > 0) || !(ti1 > ti0) || !(x_max_D > 0) ||
        !(r_max_R > 0))
        return wg_fail(WG_ERR_INVALID, "wg_set_deficit_table: null pointer or bad grid");
    if ((long long)n_ct * n_ti * n_x * n_r >= (1ll << 30)) return wg_fail(WG_ERR_INVALID, "wg_set_deficit_table: table too large");
    WG_HIPCHK(hipSetDevice(h->device));
    WG_HIPCHK(hipDeviceSynchronize());
    drop_step_graphs(h);
    FlowP& f = h->fp;
    h->fd.dtab = table_dev;            // borrowed: the caller keeps the buffer alive
    f.an_ct = n_ct; f.an_ti = n_ti; f.an_x = n_x; f.an_r = n_r;
    f.an_ct0 = (float)ct0; f.an_inv_dct = (float)((n_ct - 1) / (ct1 - ct0));
    f.an_lti0 = (float)std::log(ti0); f.an_inv_dlti = (float)((n_ti - 1) / (std::log(ti1) - std::log(ti0)));
    f.an_inv_dx = (float)((n_x - 1) / x_max_D); f.an_inv_dr = (float)((n_r - 1) / r_max_R);
    return 0;
}

extern "C" int wg_set_turbulence_box(wg_handle h, const float* box_dev, int nx, int ny, int nz, double dx,
                                     double dy, double dz) {
    const float* one[1] = {box_dev};
    if (!box_dev) return wg_fail(WG_ERR_INVALID, "turbulence box: null pointer or bad dimensions");
    return wg_set_turbulence_boxes(h, one, 1, nx, ny, nz, dx, dy, dz);
}

extern "C" int wg_set_wind(wg_handle h, const double* wind_host) {
    if (!h) return wg_fail(WG_ERR_INVALID, "null handle");
    WG_HIPCHK(hipSetDevice(h->device));
    WG_HIPCHK(hipDeviceSynchronize());
    drop_step_graphs(h);
    if (!wind_host) { h->d.wind_override = nullptr; return sync_dev_params(h); }
    if (!h->wind_dev) {
        double* w = nullptr;
        int rc = dev_alloc(h, &w, (size_t)h->p.B * 3, false);
        if (rc) return rc;
        h->wind_dev = w;
    }
    WG_HIPCHK(hipMemcpy(h->wind_dev, wind_host, sizeof(double) * 3 * (size_t)h->p.B, hipMemcpyHostToDevice));
    h->d.wind_override = h->wind_dev;
    return sync_dev_params(h);
}

extern "C" int wg_set_box_ids(wg_handle h, const int32_t* ids_host) {
    if (!h) return wg_fail(WG_ERR_INVALID, "null handle");
    WG_HIPCHK(hipSetDevice(h->device));
    WG_HIPCHK(hipDeviceSynchronize());
    drop_step_graphs(h);
    if (!ids_host) { h->d.box_override = nullptr; return sync_dev_params(h); }
    // (a caller error must not produce results labelled with the wrong box: wg_ctx_init would fold a bad id to box 0 and
    // ignores the table without a pool)
    if (h->p.turb_mode != WG_TURB_BOX_POOL || h->p.n_boxes < 1)
        return wg_fail(WG_ERR_INVALID, "wg_set_box_ids: the handle has no box pool (turb_mode WG_TURB_BOX_POOL + wg_set_turbulence_boxes first)");
    for (int b = 0; b < h->p.B; ++b)
        if (ids_host[b] >= h->p.n_boxes)
            return wg_fail(WG_ERR_INVALID, "wg_set_box_ids: env " + std::to_string(b) + " asks for box " + std::to_string(ids_host[b]) +
                                            " of a pool of " + std::to_string(h->p.n_boxes));
    if (!h->box_ids_dev) {
        int* w = nullptr;
        int rc = dev_alloc(h, &w, (size_t)h->p.B, false);
        if (rc) return rc;
        h->box_ids_dev = w;
    }
    WG_HIPCHK(hipMemcpy(h->box_ids_dev, ids_host, sizeof(int) * (size_t)h->p.B, hipMemcpyHostToDevice));
    h->d.box_override = h->box_ids_dev;
    return sync_dev_params(h);
}

extern "C" int wg_set_wind_device(wg_handle h, const double* wind_dev) {
    if (!h) return wg_fail(WG_ERR_INVALID, "null handle");
    if (h->d.wind_override != wind_dev) drop_step_graphs(h);
    h->d.wind_override = wind_dev;      // borrowed; read by wg_ctx_init (k_init / head of k_flow) in stream order
    if (int rc = wg_use_device(h->device)) return rc;
    return sync_dev_params(h);
}

extern "C" int wg_set_flow_script(wg_handle h, const float* uvw_dev, const float* power_dev, int n_rows) {
    if (!h) return wg_fail(WG_ERR_INVALID, "null handle");
    drop_step_graphs(h);
    h->d.script_uvw = uvw_dev;
    h->d.script_power = power_dev;
    h->p.script_rows = n_rows;
    h->fd.script_uvw = uvw_dev;
    h->fd.script_power = power_dev;
    h->fp.script_rows = n_rows;
    if (int rc = wg_use_device(h->device)) return rc;
    return sync_dev_params(h);
}

// The event pool is created by wg_kernel_timing(enable), i.e. outside any timed region, and is bounded: when it is
// exhausted the remaining steps of the window simply go unsampled.
static bool time_begin(wg_env_s* h, int kind, hipStream_t st) {
    if (!h->timing || h->ev_used + 2 > h->ev.size()) return false;
    h->ev_kind[h->ev_used / 2] = kind;
    hipEventRecord(h->ev[h->ev_used], st);
    return true;
}
static void time_end(wg_env_s* h, hipStream_t st) {
    hipEventRecord(h->ev[h->ev_used + 1], st);
    h->ev_used += 2;
}

extern "C" int wg_reset(wg_handle h, const uint8_t* env_mask_host, const uint64_t* seeds_host, float* obs_dev,
                        void* stream) {
    if (!h) return wg_fail(WG_ERR_INVALID, "null handle");
    hipStream_t st = (hipStream_t)stream;
    WG_HIPCHK(hipSetDevice(h->device));
    if (h->p.turb_mode >= WG_TURB_BOX && !h->d.box)
        return wg_fail(WG_ERR_INVALID, "turbtype Mann*: call wg_set_turbulence_box before wg_reset");
    if (h->fp.added && !h->fd.abox4)
        return wg_fail(WG_ERR_INVALID, "added_turbulence: call wg_set_added_turbulence_box before wg_reset");
    if (h->fp.deficit_model == 2 && !h->fd.dtab)
        return wg_fail(WG_ERR_INVALID, "deficit_model 2: call wg_set_deficit_table before wg_reset");
    const uint8_t* mask = nullptr;
    const uint64_t* seeds = nullptr;
    bool all = true;
    if (env_mask_host) {
        for (int b = 0; b < h->p.B; ++b) all = all && env_mask_host[b] != 0;
        WG_HIPCHK(hipMemcpyAsync(h->mask_dev, env_mask_host, (size_t)h->p.B, hipMemcpyHostToDevice, st));
        mask = h->mask_dev;
    }
    if (seeds_host) {
        WG_HIPCHK(hipMemcpyAsync(h->seeds_dev, seeds_host, sizeof(uint64_t) * (size_t)h->p.B, hipMemcpyHostToDevice, st));
        seeds = h->seeds_dev;
    }
    // the sticky error word is cleared only by a reset of the whole batch: a masked reset must not drop an error
    // another env latched
    if (all) WG_HIPCHK(hipMemsetAsync(h->d.status, 0, sizeof(int), st));
    wg_launch_init(&h->p, &h->d, mask, seeds, st);
    // RESET-mode launches develop the masked envs' episodes (fs.run(t_developed) + window fill).  The planned count
    // covers every episode the config's wind range can produce; a wind override (wg_set_wind / wg_set_wind_device,
    // FarmEval.set_wind_vals) may ask for a slower wind than ws_min, so the device reports how many live slots are
    // still developing and the loop goes on until none is.
    const int n_plan = h->d.script_uvw ? ((h->p.K * (std::max(h->p.fill_a, h->p.fill_b) + 1)) / h->plan.reset_chunk + 2)
                                       : h->plan.reset_launches;
    long launched = 0;
    int batch = n_plan;
    for (;;) {
        for (int i = 0; i < batch; ++i) wg_launch_flow(&h->fp, &h->fd, WG_MODE_RESET, nullptr, mask, h->plan.reset_chunk, st);
        {
            const hipError_t le = hipGetLastError();
            if (le != hipSuccess) return wg_fail(WG_ERR_HIP, std::string("wg_reset: k_flow launch failed: ") + hipGetErrorString(le));
        }
        launched += batch;
        int unready = 0;
        WG_HIPCHK(hipMemsetAsync(h->unready_dev, 0, sizeof(int), st));
        wg_launch_unready(&h->p, &h->d, mask, h->unready_dev, st);
        WG_HIPCHK(hipMemcpyAsync(&unready, h->unready_dev, sizeof(int), hipMemcpyDeviceToHost, st));
        WG_HIPCHK(hipStreamSynchronize(st));
        if (unready == 0) break;
        if (launched > 4000000L / h->plan.reset_chunk)
            return wg_fail(WG_ERR_STATE, "wg_reset: episode development does not terminate (wind speed override ~ 0?)");
        batch = std::max(8, n_plan / 4);
    }
    wg_launch_glue(&h->p, &h->d, 1, mask, obs_dev, nullptr, nullptr, nullptr, st, h->p_dev, h->d_dev);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

// one more step for wg_kernel_timing's averages -> whether this one's kernels are bracketed with timing events
static bool count_step(wg_env_s* h) {
    h->n_step_launches++;
    return h->timing && (h->timing_phase++ % h->timing_period == 0);
}

// the launches of one step(); `sample`: bracket the two kernels with timing events
static void launch_step(wg_env_s* h, const float* actions_dev, float* obs_dev, float* reward_dev, uint8_t* truncated_dev,
                        float* final_obs_dev, hipStream_t st, bool sample) {
    // step() as ONE launch (k_flow_env with the glue as its tail): sums-mode handles on the env kernel whose observation has
    // no TI / farm-level entries; a flow script (replay mode) falls back to the two launches.  (Null output pointers are
    // legal on either path: lean_step checks each one before it stores.)
    if (h->fp.env_fused && h->fd.script_uvw == nullptr) {
        if (sample) sample = time_begin(h, 0, st);
        if (h->fp.turb_mode == WG_TURB_NONE) wg_launch_step_env(&h->fp, &h->fd, &h->p, &h->d, actions_dev, obs_dev, reward_dev, truncated_dev, final_obs_dev, st);
        else wg_launch_step_envb(&h->fp, &h->fd, &h->p, &h->d, actions_dev, obs_dev, reward_dev, truncated_dev, final_obs_dev, st);
        if (sample) time_end(h, st);
        return;
    }
    if (sample) sample = time_begin(h, 0, st);
    wg_launch_flow(&h->fp, &h->fd, WG_MODE_STEP, actions_dev, nullptr, 0, st);
    if (sample) { time_end(h, st); sample = time_begin(h, 1, st); }
    wg_launch_glue(&h->p, &h->d, 0, nullptr, obs_dev, reward_dev, truncated_dev, final_obs_dev, st, h->p_dev, h->d_dev);
    if (sample) time_end(h, st);
}

extern "C" int wg_step(wg_handle h, const float* actions_dev, float* obs_dev, float* reward_dev,
                       uint8_t* truncated_dev, float* final_obs_dev, void* stream) {
    if (!h || !actions_dev || !obs_dev) return wg_fail(WG_ERR_INVALID, "null argument");
    if (int rc = wg_use_device(h->device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool sample = count_step(h);
    if (!h->graph_mode || sample) {
        launch_step(h, actions_dev, obs_dev, reward_dev, truncated_dev, final_obs_dev, st, sample);
        // a rejected launch (bad configuration, out-of-resources) must not pass for a step that returned stale outputs
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) return wg_fail(WG_ERR_HIP, std::string("wg_step: kernel launch failed: ") + hipGetErrorString(le));
        return 0;
    }
    // graph mode: one hipGraphLaunch per step.  A graph is captured once per distinct set of I/O pointers (a training
    // loop recycles a handful of action / observation buffers) on the handle's own stream — the caller's stream may be
    // the null stream, which cannot be captured — and replayed on the caller's stream.
    const void* key[5] = {actions_dev, obs_dev, reward_dev, truncated_dev, final_obs_dev};
    wg_env_s::StepGraph* g = nullptr;
    for (auto& c : h->graphs)
        if (!memcmp(c.key, key, sizeof(key))) { g = &c; break; }
    if (!g) {
        if (h->graphs.size() >= WG_MAX_STEP_GRAPHS) {      // evict the least recently used entry
            size_t lru = 0;
            for (size_t i = 1; i < h->graphs.size(); ++i)
                if (h->graphs[i].last_use < h->graphs[lru].last_use) lru = i;
            hipDeviceSynchronize();          // (the evicted exec may still be running)
            hipGraphExecDestroy(h->graphs[lru].exec);
            hipGraphDestroy(h->graphs[lru].graph);
            h->graphs.erase(h->graphs.begin() + lru);
        }
        wg_env_s::StepGraph ng;
        memcpy(ng.key, key, sizeof(key));
        // Whatever fails between Begin and End, the capture is always ended (a stream left in capture mode would break
        // every later graph-mode step) and the partial graph destroyed; the step then falls back to direct launches
        // and graph mode is switched off for the handle.
        hipError_t e = hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal);
        bool ok = e == hipSuccess;
        if (ok) {
            launch_step(h, actions_dev, obs_dev, reward_dev, truncated_dev, final_obs_dev, h->cap_stream, false);
            const hipError_t le = hipGetLastError();
            ng.graph = nullptr;
            e = hipStreamEndCapture(h->cap_stream, &ng.graph);
            ok = le == hipSuccess && e == hipSuccess && ng.graph != nullptr;
            if (ok) {
                e = hipGraphInstantiate(&ng.exec, ng.graph, nullptr, nullptr, 0);
                ok = e == hipSuccess;
            }
            if (!ok && ng.graph) hipGraphDestroy(ng.graph);
        }
        if (!ok) {
            (void)hipGetLastError();
            h->graph_mode = false;
            if (h->hooks.debug) fprintf(stderr, "[windgym] step-graph capture failed; using direct launches\n");
            launch_step(h, actions_dev, obs_dev, reward_dev, truncated_dev, final_obs_dev, st, false);
            const hipError_t le = hipGetLastError();
            if (le != hipSuccess) return wg_fail(WG_ERR_HIP, std::string("wg_step: kernel launch failed: ") + hipGetErrorString(le));
            return 0;
        }
        h->graphs.push_back(ng);
        g = &h->graphs.back();
    }
    g->last_use = ++h->graph_clock;
    WG_HIPCHK(hipGraphLaunch(g->exec, st));
    return 0;
}

extern "C" int wg_set_step_graph(wg_handle h, int enable) {
    if (!h) return wg_fail(WG_ERR_INVALID, "null handle");
    h->graph_mode = enable != 0;
    if (!h->graph_mode) drop_step_graphs(h);
    return 0;
}

extern "C" int wg_check(wg_handle h, void* stream) {
    if (!h) return wg_fail(WG_ERR_INVALID, "null handle");
    if (int rc = wg_use_device(h->device)) return rc;
    int status = 0;
    WG_HIPCHK(hipMemcpyAsync(&status, h->d.status, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    WG_HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    WG_HIPCHK(hipGetLastError());
    // (a bit mask: reported by priority — the reference treats the first two as fatal exceptions)
    if (status & WG_STATUS_BIT_NAN_POWER) return wg_fail(WG_ERR_NAN_POWER, "NaN Power");
    if (status & WG_STATUS_BIT_STATE)
        return wg_fail(WG_ERR_STATE, "step() on a truncated env without reset (or background episode not ready)");
    if (status & WG_STATUS_BIT_RANGE)
        return wg_fail(WG_ERR_RANGE, "a wake particle's emission record left its 16-bit range (k > 0.25: local TI > 0.65, or |hv| > 16 m/s: "
                            "rotor wind speed > 40 m/s) and was saturated");
    return 0;
}

extern "C" int wg_set_obs_multi_buffer(wg_handle h, float* obs_multi_dev) {
    if (!h) return wg_fail(WG_ERR_INVALID, "null handle");
    // k_glue keeps one farm block per wave in LDS for the per-agent packing (wg_launch_glue): it must fit a workgroup's
    // 64 KB by itself (the staged rings give way first)
    if (obs_multi_dev && (size_t)h->p.farm_obs * 4 * WG_NWAVES > 65536)
        return wg_fail(WG_ERR_UNSUPPORTED, "wg_set_obs_multi_buffer: the farm-level observation block is too long for the fused "
                                        "per-agent packing (use wg_obs_multi)");
    if (h->d.multi_out != obs_multi_dev) drop_step_graphs(h);
    h->d.multi_out = obs_multi_dev;     // borrowed; written by k_glue in every following wg_step / wg_reset
    if (!obs_multi_dev) h->d.multi_fin = nullptr;      // (the final buffer is written by the per-agent instantiations only)
    if (int rc = wg_use_device(h->device)) return rc;
    // (the per-agent instantiation of k_glue neither consumes nor retires the prepared first observations of
    // WgPtrs::next_obs: switching between the two must not leave a flag of an episode that has since been replaced)
    if (h->d.next_obs_ok) {
        WG_HIPCHK(hipDeviceSynchronize());
        WG_HIPCHK(hipMemset(h->d.next_obs_ok, 0, sizeof(int) * (size_t)h->p.B * 2));
    }
    return sync_dev_params(h);
}

extern "C" int wg_set_final_obs_multi_buffer(wg_handle h, float* final_obs_multi_dev) {
    if (!h) return wg_fail(WG_ERR_INVALID, "null handle");
    if (final_obs_multi_dev && !h->d.multi_out)
        return wg_fail(WG_ERR_INVALID, "wg_set_final_obs_multi_buffer: register the per-agent buffer first (wg_set_obs_multi_buffer)");
    // (same bound as wg_set_obs_multi_buffer: the farm block of a wave's agents is built once, in LDS, for both buffers)
    if (final_obs_multi_dev && (size_t)h->p.farm_obs * 4 * WG_NWAVES > 65536)
        return wg_fail(WG_ERR_UNSUPPORTED, "wg_set_final_obs_multi_buffer: the farm-level observation block is too long for the fused "
                                        "per-agent packing (use wg_obs_multi)");
    if (h->d.multi_fin != final_obs_multi_dev) drop_step_graphs(h);
    h->d.multi_fin = final_obs_multi_dev;     // borrowed; written by the glue of every following wg_step
    if (int rc = wg_use_device(h->device)) return rc;
    return sync_dev_params(h);
}

extern "C" int wg_obs_multi(wg_handle h, float* obs_dev, void* stream) {
    if (!h || !obs_dev) return wg_fail(WG_ERR_INVALID, "null argument");
    if (int rc = wg_use_device(h->device)) return rc;
    wg_launch_obs_multi(&h->p, &h->d, obs_dev, (hipStream_t)stream);
    return 0;
}

extern "C" int wg_get_measurements(wg_handle h, float* out_dev, void* stream) {
    if (!h || !out_dev) return wg_fail(WG_ERR_INVALID, "null argument");
    if (int rc = wg_use_device(h->device)) return rc;
    wg_launch_measurements(&h->p, &h->d, out_dev, (hipStream_t)stream);
    return 0;
}

extern "C" int wg_get_windspeed(wg_handle h, int env, int farm, const float* x_dev, int nx, const float* y_dev, int ny,
                                float z, int include_wakes, float* uvw_dev, void* stream) {
    if (!h || !x_dev || !y_dev || !uvw_dev) return wg_fail(WG_ERR_INVALID, "null argument");
    if (int rc = wg_use_device(h->device)) return rc;
    if (env < 0 || env >= h->p.B || farm < 0 || farm >= h->p.F) return wg_fail(WG_ERR_INVALID, "env / farm index out of range");
    if (nx <= 0 || ny <= 0 || (long long)nx * ny > (1ll << 30)) return wg_fail(WG_ERR_INVALID, "bad grid size");
    if (h->fp.script_rows > 0) return wg_fail(WG_ERR_UNSUPPORTED, "no flow field in flow-script replay mode");
    wg_launch_windspeed(&h->fp, &h->fd, env, farm, x_dev, nx, y_dev, ny, z, include_wakes, uvw_dev, (hipStream_t)stream);
    return 0;
}

extern "C" int wg_get_info(wg_handle h, wg_info_field field, void* out_dev, void* stream) {
    if (!h || !out_dev) return wg_fail(WG_ERR_INVALID, "null argument");
    if (int rc = wg_use_device(h->device)) return rc;
    if ((int)field < 0 || (int)field > WG_INFO_BOX_ID) return wg_fail(WG_ERR_INVALID, "unknown info field");
    wg_launch_info(&h->p, &h->d, (int)field, out_dev, (hipStream_t)stream);
    return 0;
}

// bytes of one wg_get_info() result (the stride of a recording in wg_rollout)
static size_t info_bytes(const wg_env_s* h, int field) {
    const size_t B = h->p.B, N = h->p.N;
    switch (field) {
    case WG_INFO_YAW_AGENT: case WG_INFO_YAW_BASE: case WG_INFO_WS_TURB: case WG_INFO_WD_TURB: case WG_INFO_POWER_TURB_AGENT:
    case WG_INFO_POWER_TURB_BASE: case WG_INFO_WS_TURB_BASE: case WG_INFO_TURB_X: case WG_INFO_TURB_Y: return B * N * 4;
    case WG_INFO_ROTOR_UVW_AGENT: case WG_INFO_ROTOR_UVW_BASE: return B * N * 3 * 4;
    case WG_INFO_WIND_F64: return B * 3 * 8;
    default: return B * 4;
    }
}

// The closed loop policy -> step -> record (windgym_hip.h: the wg_rollout* entries) exists once: rollout_loop.  An entry describes
// its call in two parts, each filled by name: the rows (RolloutRows: the env side) and what acts on them (RolloutActor).
//
// The env side: which rows the steps write and the actor reads, how many per env, what the critic reads, the messages' names.
struct RolloutRows {
    const char *who, *obs_name;    // prefix of every message; the buffer the actor reads, as the messages name it
    int per_env, width, n_out;     // actor rows per env, their width, actions per row
    int n_in;                      // the inputs a policy must map: `width`, or the hidden size of the LSTMs in front of it ...
    std::string needs;             // ... and the end of the message that says so
    const char* unready;           // non-null: refused with this message
    bool per_agent;                // the steps write the actor's rows through WgPtrs::multi_out / multi_fin, re-aimed per step
    wg_rollout_multi_bufs o;       // obs_multi / final_obs_multi: what the ACTOR reads; obs / final_obs: the steps' flat rows
    // what the CRITIC reads: v_env rows per env of v_in inputs, slots [T+1] of v_obs and [T] of v_fin (null: no final rows given,
    // named fin_name in the refusal) — the actor's own rows, or the flat rows under a centralised critic
    int v_env, v_in;
    const float *v_obs, *v_fin;
    const char* fin_name;
    // non-null: the actor's rows are NORMALISED copies of the steps' flat rows (wg_rollout_norm) — after every step the
    // observation half of this wg_norm is enqueued: o.obs[t + 1] -> o.obs_multi[t + 1], o.final_obs[t] -> o.final_obs_multi[t]
    wg_norm_s* norm;
};

// The LSTMs in front of a recurrent actor's heads (wg_rollout_lstm: `lstm`; wg_lstm_pop_rollout: `lpop`, `lstm` its member 0's) and
// the layout of their scratch [3, B, H], stated here once: the heads read the h' rows of the step — h_pi the actor, h_vf the critic,
// h_fin the critic on the final rows — and a shared LSTM's critic reads h_pi (its "critic net" is the one net it has).
struct RolloutLstm {
    wg_lstm_s* lstm;               // null: no front stage
    wg_lstm_pop_s* lpop;
    const wg_rollout_lstm_bufs* lb;
    int B, H, nets;
    bool two() const { return nets == 2; }
    size_t sH() const { return (size_t)B * H; }
    float* h_pi() const { return lb->scratch; }
    float* h_vf() const { return two() ? h_pi() + sH() : h_pi(); }
    float* h_fin() const { return h_pi() + 2 * sH(); }
};

// What acts: a step's ONE act launch (`act`, chosen by the entry), its noise, and the optional front stage.  Built by name; a
// member an entry does not name is zero.
struct RolloutActor {
    enum Act { POLICY, POPULATION, TABLE } act;
    wg_policy_s* p;                // POLICY: the policy; POPULATION: member 0, checked in every member's place; TABLE: null
    wg_pop_s* pop;                 // POPULATION: the slot table, prepared for these buffers (it carries the members' seeds and row offsets)
    wg_yaw_table_s* table;         // TABLE: k_yaw_table_act on the env's current wind and yaws; nothing is sampled or valued
    int deterministic;
    uint64_t seed, counter0, row_offset;      // (a population's entries leave seed and row_offset 0: the slot table carries the members' own)
    RolloutLstm front;
};

static int rollout_check(const wg_env_s* h, int n_steps, const RolloutRows& g, const RolloutActor& a) {
    const wg_rollout_multi_bufs& o = g.o;
    const wg_policy_s* p = a.p;
    const std::string who = std::string(g.who) + ": ";
    if (n_steps < 0) return wg_fail(WG_ERR_INVALID, who + "n_steps < 0");
    if (!o.obs_multi || !o.actions || !o.reward || !o.truncated)
        return wg_fail(WG_ERR_INVALID, who + g.obs_name + ", actions, reward and truncated buffers are required");
    if (!p) {      // (no policy: nothing of one is checked)
        if (o.raw || o.logp || o.value || o.final_value)
            return wg_fail(WG_ERR_INVALID, who + "raw, logp, value and final_value must be NULL: a yaw table samples nothing and has no critic");
    } else {
        if (p->w.device != h->device) return wg_fail(WG_ERR_INVALID, who + "policy and handle live on different devices");
        if (p->P.n_in != g.n_in || p->P.n_out != g.n_out || (p->P.n_layers[1] != 0 && p->P.n_in_vf != g.v_in))
            return wg_fail(WG_ERR_INVALID, who + "the policy maps " + std::to_string(p->P.n_in) + " -> " + std::to_string(p->P.n_out) +
                                            (p->P.n_in_vf != p->P.n_in ? " (its critic reads " + std::to_string(p->P.n_in_vf) + " inputs)" : std::string()) + g.needs);
        if (g.unready) return wg_fail(WG_ERR_INVALID, who + g.unready);
        if (!g.v_obs) return wg_fail(WG_ERR_INVALID, who + "a centralised critic reads the flat observation: obs is required (slot 0 is input)");
        if (o.final_value && !g.v_fin) return wg_fail(WG_ERR_INVALID, who + "final_value needs " + g.fin_name);
        if ((o.value || o.final_value) && p->P.n_layers[1] == 0) return wg_fail(WG_ERR_INVALID, who + "value requested from a policy without a critic");
        if (!p->P.has_log_std && (!a.deterministic || o.logp))
            return wg_fail(WG_ERR_INVALID, who + "a stochastic rollout / log-probabilities need a policy with log_std");
    }
    if (o.n_info < 0 || (o.n_info > 0 && (!o.info_fields || !o.info_out))) return wg_fail(WG_ERR_INVALID, who + "bad info arguments");
    for (int i = 0; i < o.n_info; ++i) {
        if (o.info_fields[i] < 0 || o.info_fields[i] > WG_INFO_BOX_ID) return wg_fail(WG_ERR_INVALID, who + "unknown info field");
        if (!o.info_out[i]) return wg_fail(WG_ERR_INVALID, who + "null info buffer");
    }
    return 0;
}

// A step is: the front stage (the LSTMs), ONE act launch, the step kernels with the info recordings, the after stage (the wg_norm).
// The per-agent buffers of step t are the kernel arguments of that step's launches (WgPtrs travels by value), so pointing the
// handle's two per-agent pointers at slot t on the host between launches is all "wg_set_obs_multi_buffer per step" takes: no
// device copy of the parameter block is read for them, nothing is synchronised.
static int rollout_loop(wg_env_s* h, int n_steps, const RolloutRows& g, const RolloutActor& a, void* stream) {
    const wg_rollout_multi_bufs& o = g.o;
    const RolloutLstm& f = a.front;
    hipStream_t st = (hipStream_t)stream;
    const int B = h->p.B, R = B * g.per_env, V = B * g.v_env;
    const size_t sBO = (size_t)B * h->p.obs_dim, sR = (size_t)R, sRO = sR * g.width, sRN = sR * g.n_out, sV = (size_t)V;
    float* const multi0 = h->d.multi_out;
    float* const fin0 = h->d.multi_fin;
    int rc = 0;
    // the rows the act launch reads at step t: slot t of the env side's (actor, critic, critic on the final rows), or — behind
    // a front stage — the one block of h' rows that the LSTMs fill every step
    struct { const float *pi, *vf, *fin; size_t s_pi, s_vf; } rd = {o.obs_multi, g.v_obs, g.v_fin, sRO, sV * g.v_in};
    if (f.lstm) rd = {f.h_pi(), f.h_vf(), f.h_fin(), 0, 0};
    auto lstm_step = [&](const float* x, const uint8_t* start, float* state_out, float* hp, float* hv, int net_mask) {
        return f.lpop ? wg_lstm_pop_step_(f.lpop, B, x, start, f.lb->state, state_out, hp, hv, net_mask, stream)
                      : wg_lstm_step(f.lstm, B, x, start, f.lb->state, state_out, hp, hv, net_mask, stream);
    };
    // the critic's LSTM on the final rows of step t, from the state after step t, which stays as it is -> h_fin
    auto lstm_final = [&](int t) {
        return lstm_step(o.final_obs + t * sBO, nullptr, nullptr, f.two() ? nullptr : f.h_fin(), f.two() ? f.h_fin() : nullptr, f.two() ? WG_LSTM_CRITIC : WG_LSTM_ACTOR);
    };
    if (f.lstm && f.lb->state0 && n_steps > 0) {
        const hipError_t ce = hipMemcpyAsync(f.lb->state0, f.lb->state, sizeof(float) * f.nets * 2 * f.sH(), hipMemcpyDeviceToDevice, st);
        if (ce != hipSuccess) return wg_fail(WG_ERR_HIP, std::string(g.who) + ": copy of the initial state failed: " + hipGetErrorString(ce));
    }
    for (int t = 0; t < n_steps && !rc; ++t) {
        if (f.lstm) {
            // (the final rows of step t - 1 first: they read the state that step t's launch then advances in place; the episode
            // starts of step t > 0 are read where the step before wrote them, truncated[t - 1] = what episode_start[t] will hold)
            if (o.final_value && t > 0) rc = lstm_final(t - 1);
            if (!rc)
                rc = lstm_step(o.obs_multi + t * sRO, t == 0 ? f.lb->episode_start : o.truncated + (size_t)(t - 1) * B, f.lb->state, f.h_pi(),
                               f.two() ? f.h_vf() : nullptr, f.two() ? WG_LSTM_ACTOR | WG_LSTM_CRITIC : WG_LSTM_ACTOR);
            if (rc) break;
        }
        // ONE act launch per step.  k_policy: the actor on step t's rows and, as further slots, the critic on its rows of step t and
        // final_value[t - 1] = V(final rows of step t - 1) (a row's value does not depend on what else the launch computes); the last
        // final_value by a launch of its own.  A population finds the same rows through its slot table.
        WgValueRows v[2];
        int nv = 0;
        if (o.value) v[nv++] = {rd.vf + t * rd.s_vf, o.value + t * sV, V};
        if (o.final_value && t > 0) v[nv++] = {rd.fin + (t - 1) * rd.s_vf, o.final_value + (t - 1) * sV, V};
        switch (a.act) {
        case RolloutActor::TABLE: wg_launch_yaw_table_act_(a.table, &h->p, &h->d, o.actions + t * sRN, st); break;
        case RolloutActor::POPULATION: rc = wg_pop_launch_(a.pop, 1, t > 0, t, a.deterministic, a.counter0 + (uint64_t)t, stream); break;
        case RolloutActor::POLICY:
            rc = wg_policy_eval_(a.p, R, rd.pi + t * rd.s_pi, a.deterministic, a.seed, a.counter0 + (uint64_t)t, a.row_offset * (uint64_t)g.per_env,
                                 o.actions + t * sRN, o.raw ? o.raw + t * sRN : nullptr, o.logp ? o.logp + t * sR : nullptr, v, nv, stream);
            break;
        }
        if (rc) break;
        if (g.per_agent) {
            h->d.multi_out = o.obs_multi + (t + 1) * sRO;
            h->d.multi_fin = o.final_obs_multi ? o.final_obs_multi + t * sRO : nullptr;
        }
        // (direct launches also in graph mode: T distinct pointer sets would only churn the graph cache)
        launch_step(h, o.actions + t * sRN, o.obs ? o.obs + (t + 1) * sBO : h->flat_scratch, o.reward + (size_t)t * B,
                    o.truncated + (size_t)t * B, o.final_obs ? o.final_obs + t * sBO : nullptr, st, count_step(h));
        for (int i = 0; i < o.n_info; ++i)
            wg_launch_info(&h->p, &h->d, o.info_fields[i], (char*)o.info_out[i] + (size_t)t * info_bytes(h, o.info_fields[i]), st);
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) rc = wg_fail(WG_ERR_HIP, std::string(g.who) + ": kernel launch failed: " + hipGetErrorString(le));
        if (g.norm && !rc)
            rc = wg_norm_obs(g.norm, B, o.obs + (t + 1) * sBO, o.obs_multi + (t + 1) * sRO, o.final_obs + t * sBO,
                             o.final_obs_multi + t * sRO, stream);
    }
    h->d.multi_out = multi0;      // the handle's own per-agent buffers again, on every way out (the device copies never changed)
    h->d.multi_fin = fin0;
    if (!rc && f.lstm && n_steps > 0) {      // episode_start[t + 1] = truncated[t] for every t: one contiguous block
        const hipError_t ce = hipMemcpyAsync(f.lb->episode_start + B, o.truncated, (size_t)n_steps * B, hipMemcpyDeviceToDevice, st);
        if (ce != hipSuccess) rc = wg_fail(WG_ERR_HIP, std::string(g.who) + ": copy of the episode starts failed: " + hipGetErrorString(ce));
        if (!rc && o.final_value) rc = lstm_final(n_steps - 1);
    }
    if (!rc && o.final_value && n_steps > 0) {
        const WgValueRows v = {rd.fin + (n_steps - 1) * rd.s_vf, o.final_value + (n_steps - 1) * sV, V};
        rc = a.act == RolloutActor::POPULATION ? wg_pop_launch_(a.pop, 0, 1, n_steps, 1, 0, stream)
                                               : wg_policy_eval_(a.p, 0, nullptr, 1, 0, 0, 0, nullptr, nullptr, nullptr, &v, 1, stream);
    }
    return rc;
}

// what the entries without a preparation of their own end in
static int rollout_run(wg_env_s* h, int n_steps, const RolloutRows& g, const RolloutActor& a, void* stream) {
    if (int rc = rollout_check(h, n_steps, g, a)) return rc;
    if (int rc = wg_use_device(h->device)) return rc;
    return rollout_loop(h, n_steps, g, a, stream);
}

// One actor row per env (every closed-loop entry but wg_rollout_multi): the rows the actor reads (`rows` / `fin`, named obs_name /
// fin_name) are the steps' flat rows or stand in their place; a policy maps n_in -> n_turb, or the refusal ends in `needs`
static RolloutRows env_rows(const wg_env_s* h, const wg_rollout_bufs* o, const char* who, int n_in, const std::string& needs, float* rows,
                            float* fin, const char* obs_name = "obs", const char* fin_name = "final_obs") {
    RolloutRows g = {};
    g.who = who; g.obs_name = obs_name; g.fin_name = fin_name;
    g.per_env = 1; g.width = h->p.obs_dim; g.n_out = h->p.N;
    g.n_in = n_in;
    g.needs = needs + std::to_string(n_in) + " / " + std::to_string(h->p.N);
    g.o.obs_multi = rows; g.o.final_obs_multi = fin;
    g.o.actions = o->actions; g.o.raw = o->raw; g.o.logp = o->logp; g.o.value = o->value; g.o.final_value = o->final_value;
    g.o.reward = o->reward; g.o.truncated = o->truncated; g.o.obs = o->obs; g.o.final_obs = o->final_obs;
    g.o.n_info = o->n_info; g.o.info_fields = o->info_fields; g.o.info_out = o->info_out;
    g.v_env = 1; g.v_in = n_in; g.v_obs = rows; g.v_fin = fin;
    return g;
}

// the LSTM side of a recurrent entry: lstm_bufs, and an LSTM (or the population's: `whose` words both) that reads the handle's rows
static int lstm_rows_check(const std::string& who, const wg_env_s* h, const wg_rollout_lstm_bufs* lb, int l_in, int l_device,
                           const char* reads, const char* whose) {
    if (l_in != h->p.obs_dim)
        return wg_fail(WG_ERR_INVALID, who + reads + " rows of " + std::to_string(l_in) + " inputs, the handle's obs_dim is " + std::to_string(h->p.obs_dim));
    if (l_device != h->device) return wg_fail(WG_ERR_INVALID, who + whose + " and handle live on different devices");
    if (!lb->state || !lb->episode_start || !lb->scratch) return wg_fail(WG_ERR_INVALID, who + ": lstm_bufs needs state, episode_start and scratch");
    return 0;
}

extern "C" int wg_rollout(wg_handle h, wg_policy p, int n_steps, int deterministic, uint64_t seed, uint64_t counter0,
                          uint64_t row_offset, const wg_rollout_bufs* o, void* stream) {
    if (!h || !p || !o) return wg_fail(WG_ERR_INVALID, "wg_rollout: null argument");
    const RolloutRows g = env_rows(h, o, "wg_rollout", h->p.obs_dim, ", the handle's obs_dim / n_turb are ", o->obs, o->final_obs);
    return rollout_run(h, n_steps, g, {.act = RolloutActor::POLICY, .p = p, .deterministic = deterministic, .seed = seed, .counter0 = counter0, .row_offset = row_offset}, stream);
}

// The policy on normalised rows: the actor and the critic read norm_obs / norm_final_obs, the steps write bufs->obs / final_obs,
// and the wg_norm's observation half runs after every step (its statistics move inside the loop).
extern "C" int wg_rollout_norm(wg_handle h, wg_policy p, wg_norm n, int n_steps, int deterministic, uint64_t seed, uint64_t counter0,
                               uint64_t row_offset, const wg_rollout_bufs* o, float* norm_obs_dev, float* norm_final_obs_dev, void* stream) {
    if (!h || !p || !n || !o) return wg_fail(WG_ERR_INVALID, "wg_rollout_norm: null argument");
    const int O = h->p.obs_dim;
    int n_obs = 0, n_envs = 0, n_device = 0;
    if (int rc = wg_norm_geometry_(n, &n_obs, &n_envs, &n_device)) return rc;
    if (n_obs != O || n_envs != h->p.B)
        return wg_fail(WG_ERR_INVALID, "wg_rollout_norm: the wg_norm holds statistics of " + std::to_string(n_obs) + " observation entries x " +
                                        std::to_string(n_envs) + " envs, the handle's obs_dim / n_envs are " + std::to_string(O) + " / " +
                                        std::to_string(h->p.B));
    if (n_device != h->device) return wg_fail(WG_ERR_INVALID, "wg_rollout_norm: wg_norm and handle live on different devices");
    if (!o->obs || !o->final_obs || !norm_final_obs_dev)
        return wg_fail(WG_ERR_INVALID, "wg_rollout_norm: obs, final_obs (the env's own rows) and norm_final_obs are required");
    RolloutRows g = env_rows(h, o, "wg_rollout_norm", O, ", the handle's obs_dim / n_turb are ", norm_obs_dev, norm_final_obs_dev, "norm_obs", "norm_final_obs");
    g.norm = n;
    return rollout_run(h, n_steps, g, {.act = RolloutActor::POLICY, .p = p, .deterministic = deterministic, .seed = seed, .counter0 = counter0, .row_offset = row_offset}, stream);
}

// The population in the policy's place: the checks are wg_rollout's on member 0 (the members share one architecture and device),
// the act is the population's slot table prepared for these buffers — which carries the members' seeds and row offsets: the
// loop's own are 0.
extern "C" int wg_pop_rollout(wg_handle h, wg_pop q, int n_steps, int deterministic, const uint64_t* seeds, uint64_t counter0,
                              const uint64_t* row_offsets, const wg_rollout_bufs* o, void* stream) {
    if (!h || !q || !o || !seeds) return wg_fail(WG_ERR_INVALID, "wg_pop_rollout: null argument");
    const int B = h->p.B;
    const RolloutRows g = env_rows(h, o, "wg_pop_rollout", h->p.obs_dim, ", the handle's obs_dim / n_turb are ", o->obs, o->final_obs);
    const RolloutActor a = {.act = RolloutActor::POPULATION, .p = q->pol[0], .pop = q, .deterministic = deterministic, .counter0 = counter0};
    if (int rc = rollout_check(h, n_steps, g, a)) return rc;
    if (int rc = wg_pop_shares(g.who, q->P, B, "envs", "n_envs = ", " does")) return rc;
    if (int rc = wg_use_device(h->device)) return rc;
    const WgPopOuts out = {o->actions, o->raw, o->logp, o->value, o->final_value, B};
    if (int rc = wg_pop_prepare_(q, "wg_pop_rollout", B, seeds, row_offsets, o->obs, o->final_obs, &out, stream)) return rc;
    return rollout_loop(h, n_steps, g, a, stream);
}

// what wg_yaw_table_act and wg_rollout_table refuse alike: a table for another turbine count or on another device
static int table_fits(const char* who, const wg_env_s* h, wg_yaw_table tab) {
    int N = 0, device = 0;
    if (int rc = wg_yaw_table_geometry_(tab, &N, &device)) return rc;
    if (N != h->p.N)
        return wg_fail(WG_ERR_INVALID, std::string(who) + ": tab holds yaws of " + std::to_string(N) + " turbines, the handle's n_turb is " + std::to_string(h->p.N));
    if (device != h->device) return wg_fail(WG_ERR_INVALID, std::string(who) + ": tab and handle live on different devices");
    return 0;
}

extern "C" int wg_yaw_table_act(wg_handle h, wg_yaw_table tab, float* action_out, void* stream) {
    if (!h) return wg_fail(WG_ERR_INVALID, "wg_yaw_table_act: null handle");
    if (!tab) return wg_fail(WG_ERR_INVALID, "wg_yaw_table_act: tab is null");
    if (!action_out) return wg_fail(WG_ERR_INVALID, "wg_yaw_table_act: action_out is null");
    if (int rc = table_fits("wg_yaw_table_act", h, tab)) return rc;
    if (int rc = wg_use_device(h->device)) return rc;
    wg_launch_yaw_table_act_(tab, &h->p, &h->d, action_out, (hipStream_t)stream);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

// The table in the policy's place: wg_rollout's checks of the buffers, none of a policy, and k_yaw_table_act as the act.
extern "C" int wg_rollout_table(wg_handle h, wg_yaw_table tab, int n_steps, const wg_rollout_bufs* o, void* stream) {
    if (!h || !tab || !o) return wg_fail(WG_ERR_INVALID, "wg_rollout_table: null argument");
    if (int rc = table_fits("wg_rollout_table", h, tab)) return rc;
    const RolloutRows g = env_rows(h, o, "wg_rollout_table", h->p.obs_dim, "", o->obs, o->final_obs);
    return rollout_run(h, n_steps, g, {.act = RolloutActor::TABLE, .table = tab, .deterministic = 1}, stream);
}

extern "C" int wg_rollout_multi(wg_handle h, wg_policy p, int n_steps, int deterministic, uint64_t seed, uint64_t counter0,
                                uint64_t row_offset, const wg_rollout_multi_bufs* o, void* stream) {
    if (!h || !p || !o) return wg_fail(WG_ERR_INVALID, "wg_rollout_multi: null argument");
    const int B = h->p.B, N = h->p.N, O = h->p.obs_dim, Om = h->p.obs_dim_multi;
    // central mode: the policy's critic has the flat observation's width (and not the actor's): it reads the steps' flat rows
    const bool central = p->P.n_layers[1] != 0 && p->P.n_in_vf != p->P.n_in && p->P.n_in_vf == O;
    RolloutRows g = {};
    g.who = "wg_rollout_multi"; g.obs_name = "obs_multi";
    g.per_env = N; g.width = g.n_in = Om; g.n_out = 1;
    g.needs = ", a shared per-turbine policy of this handle maps obs_dim_multi = " + std::to_string(Om) +
              " -> 1, its critic on the same " + std::to_string(Om) + " inputs (one value per agent) or on obs_dim = " +
              std::to_string(O) + " (a centralised critic: wg_policy_create_vf)";
    if (!h->d.multi_out) g.unready = "register a per-agent buffer first (wg_set_obs_multi_buffer); obs_multi[0] is what it held";
    g.per_agent = true;
    g.o = *o;
    g.v_env = central ? 1 : N; g.v_in = central ? O : Om;
    g.v_obs = central ? o->obs : o->obs_multi; g.v_fin = central ? o->final_obs : o->final_obs_multi;
    g.fin_name = central ? "final_obs (a centralised critic reads the flat rows)" : "final_obs_multi";
    const RolloutActor a = {.act = RolloutActor::POLICY, .p = p, .deterministic = deterministic, .seed = seed, .counter0 = counter0, .row_offset = row_offset};
    if (int rc = rollout_check(h, n_steps, g, a)) return rc;
    if ((long long)B * N > 0x7fffffffLL) return wg_fail(WG_ERR_UNSUPPORTED, "wg_rollout_multi: more than 2^31 agent rows");
    if (int rc = wg_use_device(h->device)) return rc;
    // the step kernels always build the flat observation: without a caller's buffer it goes to a row block of the handle's own
    // (allocated by the first call that needs it, before anything is enqueued)
    if (!o->obs && !h->flat_scratch)
        if (int rc = dev_alloc(h, &h->flat_scratch, (size_t)B * h->p.obs_dim, false)) return rc;
    return rollout_loop(h, n_steps, g, a, stream);
}

// A recurrent policy: the checks are wg_rollout's with the policy on the LSTM's hidden rows, the LSTM's launches are the front stage.
extern "C" int wg_rollout_lstm(wg_handle h, wg_lstm lstm, wg_policy p, int n_steps, int deterministic, uint64_t seed, uint64_t counter0,
                               uint64_t row_offset, const wg_rollout_bufs* o, const wg_rollout_lstm_bufs* lb, void* stream) {
    if (!h || !lstm || !p || !o || !lb) return wg_fail(WG_ERR_INVALID, "wg_rollout_lstm: null argument");
    int l_in = 0, H = 0, nets = 0, l_device = 0;
    if (int rc = wg_lstm_geometry_(lstm, &l_in, &H, &nets, &l_device)) return rc;
    if (int rc = lstm_rows_check("wg_rollout_lstm", h, lb, l_in, l_device, ": lstm reads", ": lstm")) return rc;
    if (p->P.n_layers[1] == 0) return wg_fail(WG_ERR_INVALID, "wg_rollout_lstm: p needs a critic (on the LSTM's hidden rows)");
    const RolloutRows g = env_rows(h, o, "wg_rollout_lstm", H, ": p reads the LSTM's hidden rows, and lstm's hidden size / the handle's n_turb are ", o->obs, o->final_obs);
    return rollout_run(h, n_steps, g, {.act = RolloutActor::POLICY, .p = p, .deterministic = deterministic, .seed = seed, .counter0 = counter0,
                                       .row_offset = row_offset, .front = {.lstm = lstm, .lb = lb, .B = h->p.B, .H = H, .nets = nets}}, stream);
}

// A population of recurrent policies in the pair's place: the checks are wg_rollout_lstm's on member 0 (the members share one
// architecture and device), the front stage is the members' LSTM launches, the act the heads' slot table on the h' rows.
extern "C" int wg_lstm_pop_rollout(wg_handle h, wg_lstm_pop q, int n_steps, int deterministic, const uint64_t* seeds, uint64_t counter0,
                                   const uint64_t* row_offsets, const wg_rollout_bufs* o, const wg_rollout_lstm_bufs* lb, void* stream) {
    if (!h || !q || !o || !lb || !seeds) return wg_fail(WG_ERR_INVALID, "wg_lstm_pop_rollout: null argument");
    const int B = h->p.B;
    wg_lstm_s* lstm = q->lstm[0];
    const int H = lstm->P.H;
    if (int rc = lstm_rows_check("wg_lstm_pop_rollout", h, lb, lstm->P.n_in, q->device, ": the LSTMs read", ": population")) return rc;
    const RolloutRows g = env_rows(h, o, "wg_lstm_pop_rollout", H, ": the heads read the LSTMs' hidden rows, and their hidden size / the handle's n_turb are ", o->obs,
                                   o->final_obs);
    const RolloutActor a = {.act = RolloutActor::POPULATION, .p = q->heads.pol[0], .pop = &q->heads, .deterministic = deterministic, .counter0 = counter0,
                            .front = {.lstm = lstm, .lpop = q, .lb = lb, .B = B, .H = H, .nets = lstm->P.n_nets}};
    if (int rc = rollout_check(h, n_steps, g, a)) return rc;
    if (int rc = wg_pop_shares(g.who, q->P, B, "envs", "n_envs = ", " does")) return rc;
    if (int rc = wg_use_device(h->device)) return rc;
    const WgPopOuts out = {o->actions, o->raw, o->logp, o->value, o->final_value, B};
    if (int rc = wg_lstm_pop_slots_(q, B, seeds, row_offsets, a.front.h_pi(), a.front.h_vf(), a.front.h_fin(), &out, stream)) return rc;
    return rollout_loop(h, n_steps, g, a, stream);
}

extern "C" int wg_metrics(wg_handle h, float* out_dev, int reset_after, void* stream) {
    if (!h || !out_dev) return wg_fail(WG_ERR_INVALID, "null argument");
    if (int rc = wg_use_device(h->device)) return rc;
    wg_launch_metrics(&h->p, &h->d, out_dev, reset_after, (hipStream_t)stream);
    return 0;
}

// The state blob starts with a header that identifies the handle geometry it was taken from; the payload is the
// concatenation of the handle's state allocations (a blob only makes sense for an identically configured handle).
// The host-owned wind override table (wg_set_wind) is configuration, not state: re-apply it after wg_set_state.
struct StateHeader {
    uint32_t magic;
    int32_t abi, B, N, F, P, S, K, turb_mode, block, ring_stride, fring_stride, power_avg, n_allocs;
    int32_t res, reserved0, pstride, n_boxes;      // particle-ring layout (uniform / compact rings); reserved0: always 0 (was: k_flow_duo)
    uint64_t payload;
};
static const uint32_t WG_STATE_MAGIC = 0x32474757u;   // "WGG2" (round 6: u_e lives in the packed record; blobs of the "WGGS" layout are refused)
static StateHeader state_header(const wg_env_s* h) {
    StateHeader sh;
    memset(&sh, 0, sizeof(sh));
    sh.magic = WG_STATE_MAGIC; sh.abi = WG_ABI_VERSION;
    sh.B = h->p.B; sh.N = h->p.N; sh.F = h->p.F; sh.P = h->p.P; sh.S = h->p.S; sh.K = h->p.K;
    sh.turb_mode = h->p.turb_mode; sh.block = h->fp.block; sh.ring_stride = h->p.ring_stride;
    sh.fring_stride = h->p.fring_stride; sh.power_avg = h->p.power_avg; sh.n_allocs = (int32_t)h->state_idx.size();
    sh.res = h->fp.res; sh.reserved0 = 0; sh.pstride = h->fp.pstride; sh.n_boxes = h->p.n_boxes;
    for (size_t i : h->state_idx) sh.payload += h->allocs[i].bytes;
    return sh;
}

extern "C" int wg_get_state(wg_handle h, void* blob_host, size_t* size) {
    if (!h || !size) return wg_fail(WG_ERR_INVALID, "null argument");
    const StateHeader sh = state_header(h);
    const size_t total = sizeof(StateHeader) + sh.payload;
    if (int rc = wg_blob_get("", h->device, blob_host, size, total)) return rc;
    if (!blob_host) return 0;
    char* o = (char*)blob_host;
    memcpy(o, &sh, sizeof(sh));
    o += sizeof(sh);
    for (size_t i : h->state_idx) {
        WG_HIPCHK(hipMemcpy(o, h->allocs[i].ptr, h->allocs[i].bytes, hipMemcpyDeviceToHost));
        o += h->allocs[i].bytes;
    }
    *size = total;
    return 0;
}
extern "C" int wg_set_state(wg_handle h, const void* blob_host, size_t size) {
    if (!h || !blob_host) return wg_fail(WG_ERR_INVALID, "null argument");
    const StateHeader want = state_header(h);
    const auto geometry = [&](const StateHeader& got) {
        if (!memcmp(&got, &want, sizeof(got)) && size == sizeof(StateHeader) + want.payload) return 0;
        return wg_fail(WG_ERR_INVALID, "state blob was taken from a differently configured handle (or another ABI version)");
    };
    if (int rc = wg_blob_set<StateHeader>("", h->device, blob_host, size, WG_STATE_MAGIC, "not a windgym state blob", geometry)) return rc;
    const char* o = (const char*)blob_host + sizeof(StateHeader);
    if (h->d.next_obs_ok) WG_HIPCHK(hipMemset(h->d.next_obs_ok, 0, sizeof(int) * (size_t)h->p.B * 2));      // (derived data, not in the blob)
    for (size_t i : h->state_idx) {
        WG_HIPCHK(hipMemcpy(h->allocs[i].ptr, o, h->allocs[i].bytes, hipMemcpyHostToDevice));
        o += h->allocs[i].bytes;
    }
    return 0;
}

extern "C" int wg_kernel_timing(wg_handle h, int enable, double* flow_ms_avg, double* glue_ms_avg, int* n_launches,
                                double* flow_steps_per_launch, double* particles_per_launch) {
    if (!h) return wg_fail(WG_ERR_INVALID, "null handle");
    WG_HIPCHK(hipDeviceSynchronize());
    unsigned long long fs_now = 0, pt_now = 0, ad_now = 0;
    {
        const size_t n_slots = (size_t)h->p.B * 2 * h->p.F;
        std::vector<WgSlot> slots(n_slots);
        WG_HIPCHK(hipMemcpy(slots.data(), h->d.slot, sizeof(WgSlot) * n_slots, hipMemcpyDeviceToHost));
        for (const WgSlot& s : slots) { fs_now += s.flow_count; pt_now += s.part_count; ad_now += s.add_count; }
    }
    double fsum = 0, gsum = 0;
    int nf = 0, ng = 0;
    if (h->ev_used) {
        WG_HIPCHK(hipDeviceSynchronize());
        for (size_t i = 0; i + 1 < h->ev_used; i += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]) != hipSuccess) continue;
            if (h->ev_kind[i / 2] == 0) { fsum += ms; nf++; } else { gsum += ms; ng++; }
        }
    }
    if (flow_ms_avg) *flow_ms_avg = nf ? fsum / nf : 0.0;
    if (glue_ms_avg) *glue_ms_avg = ng ? gsum / ng : 0.0;
    if (n_launches) *n_launches = nf;
    // farm flow-steps per STEP-mode launch since the last call (all launches, sampled or not)
    if (flow_steps_per_launch) *flow_steps_per_launch = h->n_step_launches ? (double)(fs_now - h->flow_steps_mark) / h->n_step_launches : 0.0;
    // particles streamed by the advection passes per launch (chain pruning makes this < farm steps x N x P);
    // the per-slot counters are 32-bit: differences stay exact as long as a slot streams < 2^32 particles per window
    // (counted on the device by the pruning-capable 256-thread variant; the others stream all N x P slots per farm step)
    if (particles_per_launch) {
        const double per_launch = h->n_step_launches ? 1.0 / h->n_step_launches : 0.0;
        *particles_per_launch = (double)(pt_now - h->particles_mark) * per_launch;
    }
    h->added_per_launch = h->n_step_launches ? (double)(ad_now - h->added_mark) / h->n_step_launches : 0.0;
    h->added_mark = ad_now;
    h->n_step_launches = 0;
    h->flow_steps_mark = fs_now;
    h->particles_mark = pt_now;
    h->ev_used = 0;
    h->timing = enable != 0;
    h->timing_period = enable > 1 ? enable : 1;
    h->timing_phase = 0;
    if (h->timing && h->ev.empty()) {          // the event pool, created here so that no timed region ever pays for it
        for (size_t i = 0; i < WG_MAX_TIMING_EVENTS; ++i) {
            hipEvent_t e;
            WG_HIPCHK(hipEventCreate(&e));
            h->ev.push_back(e);
        }
        h->ev_kind.assign(WG_MAX_TIMING_EVENTS / 2, 0);
    }
    return 0;
}

// what wg_steady_power and wg_steady_optimize check alike, and the parameter block their kernels share
static int steady_params(wg_handle h, const char* who, int model, int n_cases, SteadyP* sp) {
    const std::string w(who);
    if (model != 0 && model != 1) return wg_fail(WG_ERR_INVALID, w + ": model must be 0 (steady state of M0) or 1 (Blondel-Cathelain + Jimenez)");
    if (n_cases < 1) return wg_fail(WG_ERR_INVALID, w + ": " + (w == "wg_steady_power" ? "n_cases" : "n_cond") + " must be >= 1");
    // model 0 is documented as the steady state of THIS handle's flow model; k_steady carries the Gaussian M0 with TI folding
    // only — a handle created with another deficit / without the folding must not get Gaussian powers silently
    if (model == 0 && (h->fp.deficit_model != 0 || h->fp.no_ti_fold))
        return wg_fail(WG_ERR_UNSUPPORTED, w + ": model 0 (steady state of the handle's flow model) is implemented for the Gaussian deficit "
                                        "with wake-TI folding only; this handle uses deficit_model " + std::to_string(h->fp.deficit_model) +
                                        (h->fp.no_ti_fold ? " without TI folding" : ""));
    memset(sp, 0, sizeof(*sp));
    sp->n_cases = n_cases; sp->N = h->p.N; sp->S = h->p.S; sp->n_tab = h->p.n_tab; sp->model = model;
    sp->n_quad = model == 0 ? 48 : 20;      // quadrature of the deflection integral (steady.py's defaults)
    sp->D = h->p.D; sp->hub = h->p.hub; sp->R = 0.5f * h->p.D;
    sp->ka = h->p.ka; sp->kb = h->p.kb; sp->eps0 = h->p.eps0; sp->hill = h->p.hill;
    sp->tia = h->p.tia; sp->tib = h->p.tib; sp->tic = h->p.tic; sp->tid = h->p.tid;
    sp->cx0 = h->p.cx0; sp->cy0 = h->p.cy0;
    sp->x_pos = h->d.x_pos; sp->y_pos = h->d.y_pos; sp->rotor_dy = h->d.rotor_dy; sp->rotor_dz = h->d.rotor_dz;
    sp->tab_ws = h->d.tab_ws; sp->tab_power = h->d.tab_power; sp->tab_ct = h->d.tab_ct;
    return 0;
}

extern "C" int wg_steady_power(wg_handle h, int model, int n_cases, const float* ws_dev, const float* wd_dev, const float* ti_dev,
                               const float* yaw_dev, float* power_dev, void* stream) {
    if (!h || !ws_dev || !wd_dev || !ti_dev || !yaw_dev || !power_dev) return wg_fail(WG_ERR_INVALID, "null argument");
    SteadyP sp;
    if (int rc = steady_params(h, "wg_steady_power", model, n_cases, &sp)) return rc;
    if (int rc = wg_use_device(h->device)) return rc;
    wg_launch_steady(&sp, ws_dev, wd_dev, ti_dev, yaw_dev, power_dev, (hipStream_t)stream);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int wg_steady_optimize(wg_handle h, int model, int n_cond, const float* ws_dev, const float* wd_dev, const float* ti_dev,
                                  int refine_pass_n, int yaw_n, const double* offsets_dev, double yaw_clip, double* yaw_dev,
                                  double* power_dev, int32_t* order_dev, void* stream) {
    if (!h) return wg_fail(WG_ERR_INVALID, "null handle");
    if (yaw_n < 2 || yaw_n > 16) return wg_fail(WG_ERR_INVALID, "wg_steady_optimize: yaw_n must be 2 .. 16 (one wave per candidate), got " + std::to_string(yaw_n));
    if (refine_pass_n < 1 || refine_pass_n > 16)
        return wg_fail(WG_ERR_INVALID, "wg_steady_optimize: refine_pass_n must be 1 .. 16, got " + std::to_string(refine_pass_n));
    if (!(yaw_clip >= 0.0)) return wg_fail(WG_ERR_INVALID, "wg_steady_optimize: yaw_clip must be >= 0");
    if (!ws_dev || !wd_dev || !ti_dev || !offsets_dev || !yaw_dev)
        return wg_fail(WG_ERR_INVALID, "wg_steady_optimize: null argument (only power_dev and order_dev may be NULL)");
    SteadyP sp;
    if (int rc = steady_params(h, "wg_steady_optimize", model, n_cond, &sp)) return rc;
    if (wg_steady_srf_lds(sp.N, yaw_n) > 65536)
        return wg_fail(WG_ERR_UNSUPPORTED, "wg_steady_optimize: " + std::to_string(sp.N) + " turbines x " + std::to_string(yaw_n) +
                                        " candidates do not fit the 64 KB of LDS of a workgroup");
    if (int rc = wg_use_device(h->device)) return rc;
    wg_launch_steady_srf(&sp, ws_dev, wd_dev, ti_dev, refine_pass_n, yaw_n, offsets_dev, yaw_clip, yaw_dev, power_dev, order_dev,
                         (hipStream_t)stream);
    WG_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int wg_added_lookups(wg_handle h, double* rotor_points_per_launch) {
    if (!h || !rotor_points_per_launch) return wg_fail(WG_ERR_INVALID, "null argument");
    *rotor_points_per_launch = h->added_per_launch;
    return 0;
}

extern "C" int wg_flow_variant(wg_handle h, int* block, int* compact, int* duo) {
    if (!h) return wg_fail(WG_ERR_INVALID, "null handle");
    if (block) *block = h->fp.block;
    if (compact) *compact = h->fp.res;
    if (duo) *duo = h->fp.envw ? 2 : 0;      // 0: one farm slot per workgroup, 2: k_flow_env (one or two waves per env)
    return 0;
}

extern "C" int wg_handle_actuation_(wg_handle h, WgActuation* out) {
    if (!h || !out) return wg_fail(WG_ERR_INVALID, "null handle");
    out->B = h->p.B; out->N = h->p.N; out->action_method = h->p.action_method; out->device = h->device;
    out->yaw_min = h->p.yaw_min; out->yaw_max = h->p.yaw_max; out->yaw_step = h->p.yaw_step; out->yaw_max_d = h->p.yaw_max_d;
    return 0;
}

extern "C" int wg_algorithmic_bytes(wg_handle h, double* bytes_per_step) {
    if (!h || !bytes_per_step) return wg_fail(WG_ERR_INVALID, "null argument");
    *bytes_per_step = h->plan.alg_bytes;
    return 0;
}

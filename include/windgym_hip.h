/*
 * windgym_hip.h — C ABI of libwindgym_hip.so: the batched, MI355X-resident WindGym step() transition.
 *
 * What this boundary replaces in the reference (DTUWindEnergy/WindGym @ 2025-04-18):
 *   - the duck-typed flow-simulation object `fs` / `fs_baseline` (external DYNAMIKS DWMFlowSimulation;
 *     every call site is listed in SURVEY.md Appendix A: WindGym/Wind_Farm_Env.py:702-711, 734, 745,
 *     770-782, 793, 945, 953; rotor_avg_windspeed :485-490; power() :495, :539-540),
 *   - the sensor model `farm_mes` (WindGym/MesClass.py:354-703),
 *   - the baseline yaw controllers (WindGym/BasicControllers/BasicControllers.py:10-73),
 *   - and the body of WindFarmEnv.reset()/step() that strings them together
 *     (WindGym/Wind_Farm_Env.py:680-802, 920-1034),
 * for a batch of `n_envs` independent farms at once.  One handle == one GPU == one shard of the env axis.
 *
 * Conventions
 *   - every entry point returns 0 on success or a negative wg_status; wg_last_error() gives the message
 *     of the last failure on the calling thread.  No C++ exception crosses the boundary.
 *   - all `*_dev` pointers are DEVICE pointers owned by the caller (PyTorch tensors' data_ptr());
 *     the library owns only the state it allocates in wg_create(); nothing is allocated on the step path.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls on one handle must be
 *     stream-ordered by the caller; a handle is not thread-safe; different handles are independent.
 *   - floating point state on the device is fp32; configuration scalars are passed as double.
 *
 * The physics is "model M0" (DESIGN.md §2): DYNAMIKS itself is not available to this build
 * (SURVEY.md §0.2-0.4), so parity for the flow values is against oracle/ (a CPU restatement of M0),
 * while the glue semantics are pinned by golden vectors recorded from the reference's own code
 * (tests/golden/).
 */
#ifndef WINDGYM_HIP_H
#define WINDGYM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WG_ABI_VERSION 4

typedef enum wg_status {
    WG_OK = 0,
    WG_ERR_INVALID = -1,      /* bad argument / inconsistent config (reference: ValueError)          */
    WG_ERR_UNSUPPORTED = -2,  /* reference: NotImplementedError (ActionMethod "absolute", Track_power)*/
    WG_ERR_HIP = -3,          /* a HIP runtime call failed                                            */
    WG_ERR_NAN_POWER = -4,    /* reference: Exception("NaN Power"), Wind_Farm_Env.py:980-981           */
    WG_ERR_STATE = -5,        /* step() on a truncated env without autoreset (reference tears fs down)*/
    WG_ERR_NOMEM = -6,
    WG_ERR_RANGE = -7         /* a wake particle's emission record left the range of its 16-bit fixed-point storage
                               * (wake-growth rate k > 0.25, i.e. local TI > 0.65, or deflection speed |hv| > 16 m/s,
                               * i.e. rotor wind speed > 40 m/s, or — turbulent inflow only — a rotor wind speed above twice
                               * the episode's free-stream speed, the scale of the record's u_e field): the value was
                               * saturated; reported by wg_check                                                      */
} wg_status;

/* sensor channels, order fixed by MesClass.turb_mes.get_measurements (MesClass.py:328-351) */
enum { WG_CH_WS = 0, WG_CH_WD = 1, WG_CH_YAW = 2, WG_CH_POWER = 3, WG_N_CH = 4 };

/* one `Mes` (MesClass.py:23-125) */
typedef struct wg_channel {
    int32_t current;       /* *_current        */
    int32_t rolling_mean;  /* *_rolling_mean   */
    int32_t history_n;     /* *_history_N      */
    int32_t history_len;   /* *_history_length (deque maxlen) */
    int32_t window_len;    /* *_window_length  */
} wg_channel;

enum { WG_ACT_YAW = 0, WG_ACT_WIND = 1 };                 /* ActionMethod, Wind_Farm_Env.py:822-864 */
enum { WG_CTRL_LOCAL = 0, WG_CTRL_GLOBAL = 1 };           /* BaseController, BasicControllers.py    */
enum { WG_YAWINIT_ZEROS = 0, WG_YAWINIT_RANDOM = 1, WG_YAWINIT_DEFINED = 2 }; /* :146-162, WindEnv.py */
enum { WG_REW_BASELINE = 0, WG_REW_POWER_AVG = 1, WG_REW_NONE = 2, WG_REW_POWER_DIFF = 3 }; /* :172-194 */
enum { WG_PEN_CHANGE = 0, WG_PEN_TOTAL = 1 };             /* _action_penalty, :804-820              */
enum { WG_NOISE_NONE = 0, WG_NOISE_NORMAL = 1 };          /* farm_mes noise, MesClass.py:436-444    */
/* turbtype (:598-668): "None" -> NONE; "Random" -> RANDOM (draws a seed, :642); "MannFixed" -> BOX (the same
 * frozen box every episode, no draw, :646-657); "MannGenerate"/"MannLoad" -> BOX_SHIFT (draws a seed like :623
 * and uses it as a random horizontal offset into the one shared box instead of generating 0.8 GB per env);
 * "MannLoad" -> BOX_POOL: a pool of K boxes (the TF_* files) resident on the GPU, one drawn per episode exactly like
 * tf_file = self.np_random.choice(self.TF_files) (:614 — the same PCG64 draw as integers(0, K)). */
enum { WG_TURB_NONE = 0, WG_TURB_RANDOM = 1, WG_TURB_BOX = 2, WG_TURB_BOX_SHIFT = 3, WG_TURB_BOX_POOL = 4 };

typedef struct wg_config {
    int32_t abi_version;       /* must be WG_ABI_VERSION */
    /* ---- batch / discretisation ------------------------------------------------------------ */
    int32_t n_envs;            /* B: farms simulated by this handle                                   */
    int32_t n_turb;            /* N = nx*ny (Wind_Farm_Env.py:139)                                    */
    int32_t n_farms;           /* F: 1, or 2 when Baseline_comp (agent farm + baseline farm, :217-220)*/
    int32_t k_sub;             /* sim_steps_per_env_step = int(dt_env/dt_sim) (:105)                  */
    int32_t n_particles;       /* P: wake-particle ring slots per turbine                             */
    int32_t n_rotor_pts;       /* S: rotor quadrature points                                          */
    double dt_sim;             /* s (:102)                                                            */
    double rotor_diameter;     /* D, turbine.diameter() (:244)                                        */
    double hub_height;         /* turbine.hub_height()                                                */
    double d_particle;         /* particle spacing in D; reference hard-codes 0.2 (:116)              */
    const double* x_pos;       /* [N] layout frame (east),  Wind_Farm_Env.py:246-252                  */
    const double* y_pos;       /* [N] layout frame (north)                                            */
    const double* rotor_dy;    /* [S] quadrature offsets in the rotor plane, metres                   */
    const double* rotor_dz;    /* [S]                                                                 */
    /* ---- turbine power / Ct table (py_wake tabular turbine; linear interpolation) ------------ */
    int32_t n_tab;
    const double* tab_ws;      /* [n_tab] ascending                                                   */
    const double* tab_power;   /* [n_tab] W                                                           */
    const double* tab_ct;      /* [n_tab]                                                             */
    /* ---- yaw actuation ----------------------------------------------------------------------- */
    double yaw_min, yaw_max;   /* deg (farm.yaw_min / yaw_max)                                        */
    double yaw_step;           /* deg per sim step (:114)                                             */
    double yaw_start;          /* 15 deg: range of yaw_init "Random" (:110, :715-720)                 */
    int32_t action_method;     /* WG_ACT_*                                                            */
    int32_t base_controller;   /* WG_CTRL_*                                                           */
    int32_t yaw_init;          /* WG_YAWINIT_*                                                        */
    const double* yaw_defined; /* [N] or NULL; used with WG_YAWINIT_DEFINED (FarmEval.set_yaw_vals)   */
    /* ---- wind-condition sampling at reset (_set_windconditions, :557-568) --------------------- */
    double ws_min, ws_max, ti_min, ti_max, wd_min, wd_max;
    double n_passthrough;      /* time_max = int(t_inflow * n_passthrough) (:732)                     */
    int32_t never_truncate;    /* FarmEval.reset: time_max = 9999999 (FarmEval.py:54-61)              */
    /* ---- sensors (farm_mes ctor, :409-451) ---------------------------------------------------- */
    wg_channel ch[WG_N_CH];
    int32_t turb_ws, turb_wd, turb_ti, turb_power, farm_ws, farm_wd, farm_ti, farm_power; /* mes_level */
    double ws_scale_min, ws_scale_max;     /* 2, 25 (:440-441)                                         */
    double wd_scale_min, wd_scale_max;     /* wd_min-5, wd_max+5 (:443-444)                            */
    double ti_scale_min, ti_scale_max;     /* TI_min_mes, TI_max_mes                                   */
    double power_max;                      /* maxturbpower (:112)                                      */
    int32_t noise;                         /* WG_NOISE_*                                               */
    double noise_sigma[WG_N_CH];           /* 0, 2, 0, 0 (MesClass.py:436-439)                         */
    /* ---- reward (:866-918, :989-996) ----------------------------------------------------------- */
    int32_t reward_mode;       /* WG_REW_*                                                            */
    int32_t power_avg;         /* deque maxlen (:142-143)                                             */
    double power_scaling;
    double action_penalty;
    int32_t penalty_type;      /* WG_PEN_*                                                            */
    /* ---- reset (:722-796) ----------------------------------------------------------------------- */
    int32_t fill_steps_agent;  /* steps_on_reset (:229-240)                                           */
    int32_t fill_steps_base;   /* hist_max (:784)                                                     */
    int32_t autoreset;         /* 0: reference semantics (step after truncation is an error);         */
                               /* 1: same-step autoreset from a pre-developed next episode            */
    int32_t extra_timestep_inc;/* WindFarmEnvMulti.step increments timestep twice (WindEnvMulti.py:219)*/
    /* ---- inflow --------------------------------------------------------------------------------- */
    int32_t turb_mode;         /* WG_TURB_*                                                           */
    /* ---- model M0 constants; 0 selects the documented default -------------------- */
    double m0_ka, m0_kb;       /* k* = ka*TI + kb              (0.38, 0.004)                          */
    double m0_eps;             /* sigma0/D = eps*sqrt(beta)    (0.2)                                  */
    double m0_hill;            /* Hill-vortex deflection speed factor (0.4)                           */
    double m0_ti_a, m0_ti_b, m0_ti_c, m0_ti_d; /* Crespo-Hernandez added TI: a*ind^b*TI^c*(x/D)^d     */
    double m0_fc_scale;        /* meandering low-pass cut-off f_c = U/(fc_scale*D)   (2.0)            */
    /* ---- chain pruning -------------------------------------------------------------------------- */
    int32_t full_chains;       /* 0: a wake particle that has passed the most downstream turbine of the farm is no
                                * longer advected — it cannot reach a rotor any more, every output of step() is
                                * unchanged; 1: advect all P slots of every chain (needed only if wg_get_windspeed
                                * must be exact behind the last turbine row)                               */
    /* ---- model options (ABI 2) ------------------------------------------------------------------- */
    int32_t added_turbulence;  /* wake-added small-scale turbulence (reference: addedTurbulenceModel =
                                * [Synchronized]AutoScalingIsotropicMannTurbulence(), Wind_Farm_Env.py:618, :638, :644,
                                * :659).  0: none; 1: an isotropic unit-variance box (wg_set_added_turbulence_box) sampled
                                * at the rotor points and scaled per source wake by k_mt = km1 |dU| + km2 |d dU / d(r/R)|
                                * (Madsen et al. 2010), same advection offset as the ambient box ("Synchronized").
                                * Ignored with turb_mode NONE (the reference has no model there, :664).              */
    int32_t no_ti_fold;        /* 1: the Crespo-Hernandez added TI is NOT folded into the k of emitted particles     */
    int32_t deficit_model;     /* 0: Gaussian (north_star); 1: super-Gaussian of Blondel & Cathelain (2020);
                                * 2: tabulated eddy-viscosity deficit (Ainslie / DWM; wg_set_deficit_table)          */
    int32_t reserved0_;
    double m0_km1, m0_km2;     /* DWM added-turbulence scaling constants (0.6, 0.35); 0 selects the default          */
    double m0_sg_af, m0_sg_bf, m0_sg_cf; /* super-Gaussian order n(x) = af exp(bf x/D) + cf (3.11, -0.68, 2.41)      */
} wg_config;

typedef struct wg_env_s* wg_handle;

/* which per-env quantity wg_get_info() copies out; names = keys of WindFarmEnv._get_info (:522-555) */
typedef enum wg_info_field {
    WG_INFO_YAW_AGENT = 0,        /* "yaw angles agent"            f32[B,N] */
    WG_INFO_YAW_BASE = 1,         /* "yaw angles base"             f32[B,N] */
    WG_INFO_WS_GLOBAL = 2,        /* "Wind speed Global"           f32[B]   */
    WG_INFO_WD_GLOBAL = 3,        /* "Wind direction Global"       f32[B]   */
    WG_INFO_TI_GLOBAL = 4,        /* "Turbulence intensity"        f32[B]   */
    WG_INFO_WS_TURB = 5,          /* "Wind speed at turbines"      f32[B,N] */
    WG_INFO_WD_TURB = 6,          /* "Wind direction at turbines"  f32[B,N] */
    WG_INFO_POWER_TURB_AGENT = 7, /* "Power pr turbine agent"      f32[B,N] */
    WG_INFO_POWER_TURB_BASE = 8,  /* "Power pr turbine baseline"   f32[B,N] */
    WG_INFO_POWER_AGENT = 9,      /* "Power agent"                 f32[B]   */
    WG_INFO_POWER_BASE = 10,      /* "Power baseline"              f32[B]   */
    WG_INFO_WS_TURB_BASE = 11,    /* "Wind speed at turbines baseline" (u component) f32[B,N] */
    WG_INFO_TURB_X = 12,          /* "Turbine x positions" (flow frame)  f32[B,N] */
    WG_INFO_TURB_Y = 13,          /* "Turbine y positions"         f32[B,N] */
    WG_INFO_TIMESTEP = 14,        /* env.timestep                  i32[B]   */
    WG_INFO_TIME_MAX = 15,        /* env.time_max                  i32[B]   */
    WG_INFO_FS_TIME = 16,         /* fs.time                       f32[B]   */
    WG_INFO_EPISODE = 17,         /* episodes completed so far     i32[B]   */
    WG_INFO_ROTOR_UVW_AGENT = 18, /* fs.windTurbines.rotor_avg_windspeed  f32[B,N,3] */
    WG_INFO_ROTOR_UVW_BASE = 19,  /* fs_baseline ...                      f32[B,N,3] */
    WG_INFO_RATED_POWER = 20,     /* turbine.power(ws) (:700)      f32[B]   */
    WG_INFO_WIND_F64 = 21,        /* (ws, wd, ti) as sampled, in double precision  f64[B,3] */
    /* farm power of the step just taken, BEFORE a same-step autoreset swapped the next episode in: what
     * infos["Power agent"] of a vector env must carry so that RecordEpisodeVals (wrappers/recordEpisodeVals.py:43-46)
     * adds the terminal step's power to the episode that ended.  Equal to POWER_AGENT / POWER_BASE for envs that did
     * not truncate.                                                                                            */
    WG_INFO_STEP_POWER_AGENT = 22, /* f32[B] */
    WG_INFO_STEP_POWER_BASE = 23,  /* f32[B] */
    WG_INFO_BOX_ID = 24            /* index of the turbulence box the running episode drew from the pool  i32[B] */
} wg_info_field;

/* number of floats of the episode-metric vector produced by wg_metrics (the all-reduce payload;
 * distributed form of wrappers/recordEpisodeVals.py:31-64 and of the WindFarmMonitor callback) */
#define WG_N_METRICS 8
enum {
    WG_MET_EP_RETURN_SUM = 0, WG_MET_EP_LENGTH_SUM = 1, WG_MET_EP_MEAN_POWER_SUM = 2, WG_MET_N_EPISODES = 3,
    WG_MET_STEP_REWARD_SUM = 4, WG_MET_FARM_POWER_SUM = 5, WG_MET_BASE_POWER_SUM = 6, WG_MET_N_STEPS = 7
};

const char* wg_last_error(void);
int wg_abi_version(void);

/* Build a batch of farms on HIP device `device`.  Host arrays referenced by cfg are copied.            */
int wg_create(const wg_config* cfg, int device, wg_handle* out);
int wg_destroy(wg_handle h);

/* Sizes derived from the config: observation length O (farm_mes.observed_variables, MesClass.py:610-618)
 * and the per-agent observation length of the PettingZoo facade as actually produced by
 * WindFarmEnvMulti._get_obs_multi (WindEnvMulti.py:79-103).                                          */
int wg_obs_dim(wg_handle h, int* obs_dim, int* obs_dim_multi);
int wg_hist_max(wg_handle h, int* hist_max);

/* Shared frozen-turbulence box for turb_mode BOX / BOX_SHIFT: 3 (u,v,w) planes of nx*ny*nz fp32 (z fastest),
 * unit variance of u; spacing in metres.  The library makes its own interleaved copy (the caller's buffer may be
 * released afterwards).  Must be called before wg_reset in the box modes.                               */
int wg_set_turbulence_box(wg_handle h, const float* box_dev, int nx, int ny, int nz,
                          double dx, double dy, double dz);

/* Evaluation over several turbulence boxes (AgentEval.eval_multiple's `turbbox` loop, AgentEval.py:579-617, through
 * FarmEval.update_tf(path): TF_files = [path], FarmEval.py:86-90): env e uses box ids_host[e] of the pool at every
 * following reset instead of drawing one (a list of one consumes no random number); < 0 = draw; NULL removes the table. */
int wg_set_box_ids(wg_handle h, const int32_t* ids_host);

/* Isotropic box of the wake-added turbulence (wg_config.added_turbulence = 1): 3 planes like above, unit variance;
 * the reference's default is hipersim's L = 5 m, Gamma = 0, 128^3 cells of 3 m
 * (examples/longer_steps_example.py:153).  The library keeps an interleaved copy.  Must be set before wg_reset.   */
int wg_set_added_turbulence_box(wg_handle h, const float* box_dev, int nx, int ny, int nz,
                                double dx, double dy, double dz);

/* Pool of n_boxes frozen boxes of equal shape for turb_mode BOX_POOL (turbtype "MannLoad": one of the TF_* files per
 * reset, Wind_Farm_Env.py:611-618).  boxes_dev: HOST array of n_boxes DEVICE pointers, each 3 planes like above.  The
 * library keeps its own interleaved copies (n_boxes x 1.07 GB for the reference's 2048 x 512 x 64 boxes — sized for
 * 288 GB of HBM).  wg_set_turbulence_box is the pool of one.                                                */
int wg_set_turbulence_boxes(wg_handle h, const float* const* boxes_dev, int n_boxes, int nx, int ny, int nz,
                            double dx, double dy, double dz);

/* Evaluation sweeps (FarmEval.set_wind_vals for a whole batch, FarmEval.py:63-78): fix the wind conditions of
 * env b to wind_host[b] = (ws, wd, ti) for every following episode; NaN entries keep the sampled value.  The env's
 * generator still consumes its draws, so seeds stay aligned.  NULL removes the override.                  */
int wg_set_wind(wg_handle h, const double* wind_host /*[B,3]*/);

/* The same with a caller-owned DEVICE buffer f64[B,3] that is read (stream-ordered) whenever an episode of env b is
 * initialised — the caller may rewrite it between steps.  This is how site-based sampling (`sample_site`,
 * WindFarmEnv._set_windconditions / _sample_site, Wind_Farm_Env.py:569-594: wd from the sector frequencies, ws from
 * the sector's Weibull, both clipped to the env's ranges; TI stays uniform = NaN here) is fed to a running batch
 * without host synchronisation.  NULL removes the override.                                                 */
int wg_set_wind_device(wg_handle h, const double* wind_dev /*[B,3]*/);

/* Test hook ("replay mode"): replace the flow physics of both farms by scripted tables so that the glue can
 * be checked against golden vectors recorded from the reference.  uvw_dev: f32[F,T,B,N,3], power_dev:
 * f32[F,T,B,N]; every flow sub-step of farm f in env b consumes row cursor[f,b]++ .  NULL disables.     */
int wg_set_flow_script(wg_handle h, const float* uvw_dev, const float* power_dev, int n_rows);

/* reset(): WindFarmEnv.reset (:680-802) for the envs whose mask byte is non-zero (NULL = all).
 * seeds: host array [B] of uint64 or NULL.  seeds[b] == UINT64_MAX keeps env b's generator running
 * (gymnasium reset(seed=None)); otherwise the env's PCG64 generator is re-seeded exactly like
 * gymnasium's np_random (np.random.default_rng(seed)).  Outputs may be NULL.
 * With autoreset on, a reset initialises BOTH episode contexts of a masked env — the episode that starts now and the
 * look-ahead episode that is developed in the background — so it consumes two episodes' worth of draws from the env's
 * generator: episode k of an env always uses draws k of its stream (one draw set per episode, in order), but an explicit
 * reset(seed=None) in the middle of an autoreset run discards the look-ahead episode that was already drawn, i.e. the
 * stream then runs one episode ahead of a reference env that was reset at the same moments.  A wind override set after
 * a reset is seen from the episode after the look-ahead one.  The sensor-noise stream is keyed by (env seed, episode
 * index, push index): an explicit reset starts a new episode index, so noise sequences are not replayed.   */
int wg_reset(wg_handle h, const uint8_t* env_mask_host, const uint64_t* seeds_host,
             float* obs_dev /*[B,O]*/, void* stream);

/* step(): WindFarmEnv.step (:920-1034) for all envs.  actions_dev f32[B,N] in [-1,1].
 * obs_dev f32[B,O] (after autoreset: first observation of the next episode), reward_dev f32[B],
 * truncated_dev u8[B]; final_obs_dev f32[B,O] or NULL receives the last observation of the episode that
 * ended (== obs for envs that did not truncate).  Asynchronous on `stream`.                            */
int wg_step(wg_handle h, const float* actions_dev, float* obs_dev, float* reward_dev,
            uint8_t* truncated_dev, float* final_obs_dev, void* stream);

/* step() as ONE graph launch: with enable != 0 the kernels of a step are captured once per
 * distinct set of I/O pointers into a HIP graph (at most 32 sets are cached, least recently used evicted) and every
 * following wg_step is a single hipGraphLaunch on the caller's stream.  Results are identical to the direct launches.
 * Setters that change kernel arguments (turbulence box, wind override, flow script, obs-multi buffer) drop the cached
 * graphs.  Default: off (two direct launches; measured faster on the host for a two-kernel step — DESIGN.md §4.4);
 * the environment variable WG_STEP_GRAPH=1 switches it on at wg_create.                                   */
int wg_set_step_graph(wg_handle h, int enable);

/* step() is asynchronous, so the errors the reference raises inside step() (Exception("NaN Power"), stepping
 * a torn-down env) are latched in a sticky device word.  wg_check synchronises `stream` and returns it
 * (0, WG_ERR_NAN_POWER, WG_ERR_STATE or WG_ERR_RANGE — the conditions are latched independently and the most serious one
 * is reported, in that order); a wg_reset of the whole batch clears it.                                                     */
int wg_check(wg_handle h, void* stream);

/* Per-agent observations of the PettingZoo facade for the current state: f32[B,N,obs_dim_multi].      */
int wg_obs_multi(wg_handle h, float* obs_dev, void* stream);

/* The same, fused into the step: once a caller-owned buffer f32[B,N,obs_dim_multi] is registered, every following
 * wg_step / wg_reset also writes the per-agent observations there (the values wg_obs_multi would return right
 * after the call) — WindFarmEnvMulti.step calls _get_obs_multi every step (WindEnvMulti.py:188-227).  NULL stops. */
int wg_set_obs_multi_buffer(wg_handle h, float* obs_multi_dev);

/* The per-agent observation an episode ENDED in (what a value bootstrap at truncation needs; the buffer above only ever
 * holds the first observation of the next episode): a second caller-owned buffer f32[B,N,obs_dim_multi].  After every
 * following wg_step, row (e, i) holds agent i's observation of the state the step ended in — for an env that truncated, the
 * FINISHED episode's (its turbine block ++ the agents' farm block, as wg_obs_multi would have returned it before the
 * reset); for every other env, bit for bit the row of the buffer above.  Needs that buffer registered (WG_ERR_INVALID
 * otherwise; unregistering it drops this one too); same length bound.  Not written by wg_reset.  NULL stops, and a handle
 * that never registered one computes exactly what it always did.                                                    */
int wg_set_final_obs_multi_buffer(wg_handle h, float* final_obs_multi_dev);

/* Unscaled, unclipped sensor values of the running episodes in the layout of the observation: f32[B,O]
 * (farm_measurements.get_*_turb() / get_*_farm(), the "... measured" entries of _get_info :529-537).   */
int wg_get_measurements(wg_handle h, float* out_dev, void* stream);

/* Flow-field view of ONE farm (0 = agent, 1 = baseline) of ONE env: (u, v, w) at the nx x ny points
 * (x_dev[i], y_dev[j], z) of the flow frame -> uvw_dev f32[3, nx, ny].  Replaces
 * fs.get_windspeed(XYView(z=hub_height, x=a, y=b), include_wakes=True) behind WindFarmEnv._render_frame /
 * init_render (Wind_Farm_Env.py:1040-1083, :464-476; AgentEval.py:220-228).                               */
int wg_get_windspeed(wg_handle h, int env, int farm, const float* x_dev, int nx, const float* y_dev, int ny,
                     float z, int include_wakes, float* uvw_dev, void* stream);

/* Lazy info dict: copy one field to out_dev (dtype/shape per wg_info_field).                           */
int wg_get_info(wg_handle h, wg_info_field field, void* out_dev, void* stream);

/* Episode-metric partial sums of this shard since the last call with reset_after != 0: f32[WG_N_METRICS]
 * in device memory (ready for one RCCL all-reduce(sum)).                                              */
int wg_metrics(wg_handle h, float* out_dev, int reset_after, void* stream);

/* Checkpoint / golden replay: serialise the full device state.  Call with blob_host == NULL to get size.  The blob
 * carries a header (magic, ABI version, batch geometry); wg_set_state rejects a blob taken from a differently
 * configured handle.  The wind override of wg_set_wind is configuration, not state (re-apply it after a restore). */
int wg_get_state(wg_handle h, void* blob_host, size_t* size);
int wg_set_state(wg_handle h, const void* blob_host, size_t size);

/* HIP-event timing of the step kernels on the stream they were launched on: average milliseconds per
 * launch of the dominant flow kernel and of the glue kernel since the last call, and the average number of
 * farm flow-steps one flow launch executed (live farms + background episode development) — the unit
 * count behind bench.py's roofline; particles_per_launch = wake particles the advection passes actually streamed
 * (chain pruning: particles behind the last turbine are not touched).  enable = 0 stops; enable = n >= 1 records events around every n-th
 * wg_step (an event pair per launch costs a few percent of a ~200 us step).                            */
int wg_kernel_timing(wg_handle h, int enable, double* flow_ms_avg, double* glue_ms_avg, int* n_launches,
                     double* flow_steps_per_launch, double* particles_per_launch);

/* deficit_model 2: the wake-deficit table the flow kernels sample instead of the Gaussian — what the reference's
 * particleDeficitGenerator=jDWMAinslieGenerator() (Wind_Farm_Env.py:706, :774) solves inside DYNAMIKS, solved on the host
 * (windgym_amd/ainslie.py restates the published DWM eddy-viscosity model).  table_dev: f32[n_ct][n_ti][n_x][n_r], the deficit
 * fraction 1 - U / U0 at Ct uniform in [ct0, ct1], ambient TI log-uniform in [ti0, ti1], x / D uniform in [0, x_max_D],
 * r / R uniform in [0, r_max_R] (linear between nodes; 0 from half a node inside r_max_R on).  Borrowed: the buffer must outlive the handle.  Before wg_reset.          */
int wg_set_deficit_table(wg_handle h, const float* table_dev, int n_ct, double ct0, double ct1, int n_ti, double ti0, double ti1,
                         int n_x, double x_max_D, int n_r, double r_max_R);

/* Mann spectral-tensor turbulence box generated on the device — MannTurbulenceField.generate(alphaepsilon, L, Gamma, Nxyz,
 * dxyz, seed) of hipersim / dynamiks behind turbtype "MannFixed" / "MannGenerate" (Wind_Farm_Env.py:624-637, :649-658;
 * tests/test_basics.py:38-45).  box_dev: f32[3][nx][ny][nz] (z fastest: what wg_set_turbulence_box takes), normalised to
 * unit standard deviation of u (the reference rescales with scale_TI(TI, U); the kernels multiply by TI * U per env).
 * noise_dev: optional complex white noise f32[3][nx][ny][nz][2] (E|n|^2 = 1) to use instead of the built-in Philox stream
 * keyed by `seed` — lets a test feed the identical noise to a CPU restatement.  Sheared von Karman tensor per wave-number
 * cell in a HIP kernel, three in-place inverse C2C transforms in hipFFT, synchronous on `stream`.  No handle needed.   */
int wg_generate_mann_box(int device, float* box_dev, int nx, int ny, int nz, double dx, double dy, double dz,
                         double alphaepsilon, double L, double Gamma, uint64_t seed, const float* noise_dev, void* stream);

/* Host only: the eddy-lifetime factor beta(kL) = Gamma (kL)^(-2/3) / sqrt(2F1(1/3, 17/6; 4/3; -(kL)^-2)) (Mann 1998) on n
 * log-spaced points kL = 10^[log10_lo, log10_hi] — the table wg_generate_mann_box interpolates (4096 points over
 * [1e-6, 1e6]); exported so that tests pin it against an independent 2F1.                                               */
int wg_mann_beta_table(double Gamma, int n, double log10_lo, double log10_hi, double* beta_out);

/* Steady-state farm power for a batch of cases — the inner loop of PyWakeAgent.yaw_optimizer_srf_vect
 * (WindGym/Agents/PyWakeAgent.py:144-288: every Serial-Refine step evaluates the farm power of yaw_n candidate yaw vectors
 * per wind condition): power_dev f32[n_cases][n_turb] (W) for ws / wd / ti f32[n_cases] and yaw_dev f32[n_cases][n_turb]
 * (degrees, flow frame).  Layout, turbine table, rotor points and model constants are the handle's.
 * model 0: the steady state of the env's own flow model (what wg_step converges to under constant yaws) — the Gaussian
 *          deficit with wake-TI folding; WG_ERR_UNSUPPORTED on a handle created with another deficit_model / no_ti_fold;
 * model 1: the reference agent's py_wake model restated from the publications (Blondel & Cathelain 2020 super-Gaussian
 *          at the rotor centre, linear superposition, Jimenez deflection, Ct cos^2(yaw)).  One kernel launch (k_steady).   */
int wg_steady_power(wg_handle h, int model, int n_cases, const float* ws_dev, const float* wd_dev, const float* ti_dev,
                    const float* yaw_dev, float* power_dev, void* stream);

/* The whole Serial-Refine yaw optimisation (WindGym/Agents/PyWakeAgent.py:144-288, yaw_optimizer_srf_vect) of n_cond wind
 * conditions in ONE kernel launch (k_steady_srf: one workgroup per condition, yaw_n waves), enqueued on `stream` without a
 * host synchronisation; ws / wd / ti f32[n_cond] may have been written earlier on the same stream.  models as wg_steady_power.
 * With P(yaw) = the sum over the turbines, in index order and in double precision, of the powers wg_steady_power returns for
 * (ws, wd, ti, (float) yaw):  yaw = 0, best = P(yaw);  for pass r < refine_pass_n, for every turbine t from upstream to
 * downstream (k_steady's order: rank by fp32 flow-frame x, ties by index):  candidates yaw_j = yaw with yaw_j[t] = yaw[t] +
 * offsets_dev[r][j] (f64[refine_pass_n][yaw_n], degrees; the add in double);  j* = the first j with the largest P(yaw_j);  if
 * P(yaw_j*) > best, yaw = yaw_j* and best = P(yaw_j*).  Outputs: yaw_dev f64[n_cond][n_turb] = yaw clamped to +-yaw_clip,
 * power_dev f64[n_cond] = best (may be NULL), order_dev i32[n_cond][n_turb] = the visiting order (may be NULL).
 * Limits: 2 <= yaw_n <= 16, 1 <= refine_pass_n <= 16.                                                                    */
int wg_steady_optimize(wg_handle h, int model, int n_cond, const float* ws_dev, const float* wd_dev, const float* ti_dev,
                       int refine_pass_n, int yaw_n, const double* offsets_dev, double yaw_clip, double* yaw_dev,
                       double* power_dev, int32_t* order_dev, void* stream);

/* Rotor points at which one flow launch looked the wake-added turbulence box up (8 corners x (u, v, w) = 96 bytes each:
 * only the rotors of targets with a candidate source wake do), averaged over the window the LAST wg_kernel_timing call
 * closed — the a7 term of bench.py's algorithmic bytes.  0 without wg_config.added_turbulence.
 * Steady inflow on the one-wave-per-env kernel (wg_flow_variant: 2; no such lookups exist there): the same word counts the
 * wake particles the advection passes actually touched per launch — moving chains whole, resting chains their new particles —
 * the numerator of bench.py's roofline.frac_touched.                                                                          */
int wg_added_lookups(wg_handle h, double* rotor_points_per_launch);

/* Algorithmic HBM bytes one wg_step() moves (the figure bench.py's roofline uses).       */
int wg_algorithmic_bytes(wg_handle h, double* bytes_per_step);

/* Which flow kernel the handle launches (diagnostics / tests; chosen in wg_create from the farm geometry and the inflow; the
 * hooks WG_FLOW_BLOCK (64 / 256) / WG_FLOW_RES (0) / WG_FLOW_ENV / WG_ENV_WPE / WG_STEP_FUSED override it among the kernels that
 * are built, honoured only with WG_DEBUG_HOOKS=1): threads per wave-group (64 or 256), 1 = compact per-turbine rings with pair-major deficit phases, and the farm
 * slots one wave serves: 0 = one (k_flow), 2 = every slot of an env / of one of its
 * contexts (k_flow_env: one or two waves per env; with the lean glue, wg_step is then ONE kernel launch).                     */
int wg_flow_variant(wg_handle h, int* block, int* compact, int* duo);

/* ---------------------------------------------------------------------------------------------------------------
 * Learned policies on the device.  The reference evaluates a stable-baselines3 model on the host, one env at a time:
 * `model.predict(obs, deterministic=...)[0]` every step of AgentEval.eval_single_fast (WindGym/AgentEval.py:179-190;
 * examples/Example 2 Evaluate pretrained agent.ipynb: PPO.load("PPO_2975000")), and trains it through SB3's rollout
 * collection (examples/longer_steps_example.py:212-240).  Here the policy is an MLP actor(-critic) evaluated by ONE kernel
 * (k_policy, windgym_amd/csrc/wg_policy.hip) on device-resident observation rows, and wg_rollout alternates it with the
 * step kernels without returning to the caller.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct wg_policy_s* wg_policy;
enum { WG_ACTV_TANH = 0, WG_ACTV_RELU = 1 };              /* SB3 MlpPolicy activation_fn: nn.Tanh (default) / nn.ReLU */
#define WG_POLICY_MAX_HIDDEN 4

/* Architecture of SB3's MlpPolicy with separate actor / critic nets (net_arch=dict(pi=[...], vf=[...]), SB3 >= 2.0):
 * actor n_in -> hidden_pi... -> n_out, critic n_in -> hidden_vf... -> 1, state-independent log_std[n_out].
 * Bounds (WG_ERR_UNSUPPORTED outside): n_in <= 2048, n_out <= 128, 0-4 hidden layers per net, widths <= 256.     */
typedef struct wg_policy_desc {
    int32_t n_in, n_out, activation;
    int32_t n_hidden_pi, hidden_pi[WG_POLICY_MAX_HIDDEN];
    int32_t n_hidden_vf, hidden_vf[WG_POLICY_MAX_HIDDEN];   /* n_hidden_vf < 0: no critic          */
    int32_t has_log_std;                                     /* 0: deterministic use only, no logp  */
} wg_policy_desc;

/* PPO.load's counterpart (AgentEval.py:179-190 needs nothing else of the model): an empty policy of the given
 * architecture on `device` (all parameters 0 until wg_policy_set_params).                                          */
int wg_policy_create(const wg_policy_desc* d, int device, wg_policy* out);
/* The same with a critic of its own input width, n_in_vf -> hidden_vf... -> 1 (1 <= n_in_vf <= 2048; the descriptor must have a
 * critic): a SPLIT policy, whose critic reads other rows than its actor — the centralised critic of multi-agent PPO (MAPPO:
 * the actor on each agent's observation, the critic on the env's flat one; wg_rollout_multi, wg_ppo_grad_shared).  The flat
 * vector keeps its order, the critic's first W is [h][n_in_vf].  wg_policy_create(d, ...) is this with n_in_vf = d->n_in.  */
int wg_policy_create_vf(const wg_policy_desc* d, int32_t n_in_vf, int device, wg_policy* out);
int wg_policy_destroy(wg_policy p);

/* All parameters as ONE flat f32 vector of wg_policy_n_params floats: actor hidden layers in order, each W [out][in]
 * row-major (torch.nn.Linear.weight) then b [out]; actor head W [n_out][.], b; critic hidden layers, critic head W [1][.],
 * b [1] (with a critic); log_std [n_out] (with has_log_std) — SB3's mlp_extractor.policy_net.*, action_net.*,
 * mlp_extractor.value_net.*, value_net.*, log_std.  `params` is a host (on_device = 0; must stay valid until the stream
 * reaches the copy) or device pointer; stream-ordered copy + repack into the kernel's layout, no synchronisation.  With a
 * device pointer this is also how a trainer pushes the weights after an optimiser step
 * (examples/longer_steps_example.py:232-240: model.learn).                                                         */
int wg_policy_set_params(wg_policy p, const float* params, size_t n, int on_device, void* stream);
int wg_policy_n_params(wg_policy p, size_t* n);

/* model.predict(obs, deterministic)[0] (AgentEval.py:179-190) for n_rows observation rows obs_dev f32[n_rows, n_in], plus what
 * SB3's rollout collection takes from policy.forward (examples/longer_steps_example.py:212-240):
 *   mean = actor(obs); raw = mean (deterministic) or mean + exp(log_std) * eps, eps ~ N(0, 1) from Philox4x32-10 keyed by
 *   (seed; row + row_offset, counter, output index) — wg_policy.h writes the stream down;
 *   action_dev f32[n_rows, n_out] = clip(raw, -1, 1) (what predict() returns for a Box and wg_step expects),
 *   raw_dev    f32[n_rows, n_out] = raw (what a PPO buffer stores),
 *   logp_dev   f32[n_rows]        = sum_j (-eps_j^2 / 2 - log_std_j - log(2 pi) / 2)  (deterministic: the density at the mean),
 *   value_dev  f32[n_rows]        = critic(obs).
 * Every output may be NULL; a net none of whose outputs is requested is not evaluated.  fp32, bit-identical from run to run,
 * and a row's outputs do not depend on n_rows or on the other rows: a batch sharded with row_offset = first global row
 * computes what the unsharded batch computes.  Row-generic: a parameter-shared per-turbine policy on the buffer of
 * wg_set_obs_multi_buffer is n_rows = B * N, n_out = 1.  One launch, asynchronous on `stream`, allocates and synchronises
 * nothing (legal inside a stream capture).  On a split policy (wg_policy_create_vf, n_in_vf != n_in) a call that asks for an
 * actor output reads rows of n_in, a call that asks for the value alone reads obs_dev f32[n_rows, n_in_vf]; the actor's outputs
 * are bit-identical to those of an equal-width policy holding the same actor parameters.  WG_ERR_INVALID: a stochastic call or
 * logp on a policy without log_std, a value on a policy without a critic, actor outputs AND the value from one obs_dev on a
 * split policy (the two nets read rows of different widths).                                                        */
int wg_policy_act(wg_policy p, int n_rows, const float* obs_dev, int deterministic,
                  uint64_t seed, uint64_t counter, uint64_t row_offset,
                  float* action_dev, float* raw_dev, float* logp_dev, float* value_dev, void* stream);

/* Caller-owned device buffers of wg_rollout, T = n_steps, B / N / O of the handle; NULL = not wanted where noted. */
typedef struct wg_rollout_bufs {
    float*   obs;          /* [T+1, B, O]  obs[0] is INPUT (the observation the env last returned); obs[t+1] after step t */
    float*   actions;      /* [T, B, N]    what wg_step received (clipped)                                        */
    float*   raw;          /* [T, B, N]    or NULL                                                               */
    float*   logp;         /* [T, B]       or NULL                                                               */
    float*   value;        /* [T, B]       or NULL: V(obs[t])                                                    */
    float*   final_obs;    /* [T, B, O]    or NULL (required with final_value)                                    */
    float*   final_value;  /* [T, B]       or NULL: V(final_obs[t]) — the value of the state step t ENDED in, also
                            *              when the env was reset in the same step                                */
    float*   reward;       /* [T, B]                                                                              */
    uint8_t* truncated;    /* [T, B]                                                                              */
    int32_t  n_info;       /* recorded info fields: info_out[i] is [T, <shape of wg_info_field info_fields[i]>]   */
    const int32_t* info_fields;      /* host arrays of n_info entries                                             */
    void* const*   info_out;
} wg_rollout_bufs;

/* The closed loop of AgentEval.eval_single_fast (AgentEval.py:179-212: predict, env.step, record) and of SB3's
 * collect_rollouts (examples/longer_steps_example.py:212-240) for the whole batch, n_steps steps, enqueued on `stream`
 * with no host synchronisation, no allocation and no return to the caller in between.  Buffers and the handle's state
 * afterwards are BIT-IDENTICAL to
 *     for t in 0 .. T-1:
 *         wg_policy_act(p, B, obs[t], deterministic, seed, counter0 + t, row_offset, actions[t], raw[t], logp[t], value[t])
 *         wg_step(h, actions[t], obs[t+1], reward[t], truncated[t], final_obs[t])
 *         wg_get_info(h, info_fields[i], info_out[i] + t * <size of the field>)       for every i
 *         wg_policy_act(p, B, final_obs[t], value only -> final_value[t])              if wanted
 * Its steps count for wg_metrics, wg_kernel_timing and wg_check like wg_step calls; the step kernels are launched directly
 * also when wg_set_step_graph is on.  This env never terminates (Wind_Farm_Env.py:1029): every episode ends by truncation,
 * so an advantage estimate bootstraps from final_value:  delta_t = r_t + gamma * final_value_t - value_t,
 * A_t = delta_t + gamma * lambda * (1 - truncated_t) * A_{t+1}.
 * WG_ERR_INVALID: null / missing required buffers, p's n_in != the handle's obs_dim or n_out != n_turb, policy and handle on
 * different devices, final_value without final_obs, value / final_value without a critic, stochastic without log_std, an
 * unknown info field.                                                                                              */
int wg_rollout(wg_handle h, wg_policy p, int n_steps, int deterministic, uint64_t seed, uint64_t counter0,
               uint64_t row_offset, const wg_rollout_bufs* out, void* stream);

/* Caller-owned device buffers of wg_rollout_multi, T = n_steps, B / N / O / Om = obs_dim_multi of the handle; one ROW per
 * agent (env e, turbine i) = row e * N + i; NULL = not wanted where noted.                                          */
typedef struct wg_rollout_multi_bufs {
    float*   obs_multi;        /* [T+1, B, N, Om]  obs_multi[0] is INPUT (the per-agent observation the env last returned) */
    float*   actions;          /* [T, B, N]        one yaw action per agent = what wg_step received (clipped)         */
    float*   raw;              /* [T, B, N]        or NULL                                                           */
    float*   logp;             /* [T, B, N]        or NULL                                                           */
    float*   value;            /* [T, B, N]        or NULL: V(obs_multi[t]) per agent          (central: [T, B], V(obs[t]))  */
    float*   final_obs_multi;  /* [T, B, N, Om]    or NULL (required with final_value; central: never required):
                                *                  wg_set_final_obs_multi_buffer                                      */
    float*   final_value;      /* [T, B, N]        or NULL: V(final_obs_multi[t])              (central: [T, B], V(final_obs[t])) */
    float*   reward;           /* [T, B]           the farm reward, shared by the env's agents                       */
    uint8_t* truncated;        /* [T, B]                                                                              */
    float*   obs;              /* [T+1, B, O]      or NULL: the flat observation; slot 0 is not touched
                                *                  (central: REQUIRED, slot 0 is INPUT — the flat observation the env last returned) */
    float*   final_obs;        /* [T, B, O]        or NULL                                     (central: required with final_value) */
    int32_t  n_info;           /* recorded info fields, as in wg_rollout_bufs                                         */
    const int32_t* info_fields;
    void* const*   info_out;
} wg_rollout_multi_bufs;

/* wg_rollout for ONE policy shared by the turbines (WindGym/WindEnvMulti.py: one agent per turbine, each seeing its own
 * turbine block plus the farm block, each sending one yaw action, all sharing the farm reward): `p` maps obs_dim_multi -> 1
 * and is evaluated on B * N agent rows per step.  Enqueued on `stream` with no host synchronisation, no allocation and no
 * return to the caller in between; buffers and the handle's state afterwards are BIT-IDENTICAL to
 *     for t in 0 .. T-1:
 *         wg_set_obs_multi_buffer(h, obs_multi[t+1]);  wg_set_final_obs_multi_buffer(h, final_obs_multi[t])
 *         wg_policy_act(p, B * N, obs_multi[t], deterministic, seed, counter0 + t, row_offset * N, actions[t], raw[t], logp[t], value[t])
 *         wg_step(h, actions[t], obs[t+1], reward[t], truncated[t], final_obs[t])
 *         wg_get_info(h, info_fields[i], info_out[i] + t * <size of the field>)       for every i
 *         wg_policy_act(p, B * N, final_obs_multi[t], value only -> final_value[t])    if wanted
 * after which the handle's own two per-agent buffers are registered again (they are not written).  The noise row of agent i
 * of env e is (row_offset + e) * N + i: a shard of the env axis computes what the unsharded batch computes.  Without `obs`
 * the steps' flat observation goes to a buffer of the handle's own, allocated by the first such call before anything is
 * enqueued.  Advantages: wg_gae_shared.
 *
 * CENTRAL mode — a split policy (wg_policy_create_vf) that maps obs_dim_multi -> 1 with its critic on n_in_vf = obs_dim: the
 * actor stays per agent, the critic reads the env's FLAT observation (centralised training, decentralised execution).  Same
 * struct; value / final_value are [T, B], `obs` is required with slot 0 as input, final_obs is required with final_value and
 * final_obs_multi with nothing.  Buffers and the handle's state afterwards are BIT-IDENTICAL to
 *     for t in 0 .. T-1:
 *         wg_set_obs_multi_buffer(h, obs_multi[t+1]);  wg_set_final_obs_multi_buffer(h, final_obs_multi[t])
 *         wg_policy_act(p, B * N, obs_multi[t], deterministic, seed, counter0 + t, row_offset * N, actions[t], raw[t], logp[t], NULL)
 *         wg_policy_act(p, B, obs[t], value only -> value[t])                          if wanted
 *         wg_step(h, actions[t], obs[t+1], reward[t], truncated[t], final_obs[t])
 *         wg_get_info(h, info_fields[i], info_out[i] + t * <size of the field>)       for every i
 *         wg_policy_act(p, B, final_obs[t], value only -> final_value[t])              if wanted
 * Advantages are then wg_gae on [T, B], shared by an env's agents; the update is wg_ppo_update_shared.  The mode is recognised by
 * the critic's width alone (n_in_vf != n_in and n_in_vf == obs_dim), so it needs obs_dim != obs_dim_multi: on a handle whose flat
 * and per-agent observations have one width (a farm of ONE turbine: one agent per env, nothing to centralise) every accepted
 * policy runs in per-agent mode.
 * WG_ERR_INVALID: as wg_rollout, with a policy that is neither obs_dim_multi -> 1 with its critic on obs_dim_multi (per agent)
 * nor obs_dim_multi -> 1 with its critic on obs_dim (central); final_value without final_obs_multi (central: without final_obs);
 * central mode without obs; no per-agent buffer registered on the handle.                                           */
int wg_rollout_multi(wg_handle h, wg_policy p, int n_steps, int deterministic, uint64_t seed, uint64_t counter0,
                     uint64_t row_offset, const wg_rollout_multi_bufs* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Training on the device: what `PPO("MlpPolicy", env, n_steps=2048).learn(...)` does between two rollouts
 * (examples/longer_steps_example.py:212-240, examples/curriculum.py:544-560) — advantages, the clipped-surrogate loss and
 * its gradient, gradient clipping and Adam — for the wg_policy above (windgym_amd/csrc/wg_ppo.hip).  fp32 throughout; every
 * entry is asynchronous on `stream`, synchronises nothing and is bit-identical from run to run (no float atomics; every sum
 * has an order fixed by the shapes alone).
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct wg_ppo_s* wg_ppo;

/* SB3's RolloutBuffer.compute_returns_and_advantage (longer_steps_example.py:232-240: model.learn) on wg_rollout's buffers
 * [T, B], with the bootstrap this never-terminating env needs (wg_rollout above):
 *   delta_t = r_t + gamma * final_value_t - value_t,   A_t = delta_t + gamma * lambda * (1 - truncated_t) * A_{t+1},  A_T = 0,
 *   returns_t = A_t + value_t.   One launch on the current device.                                                 */
int wg_gae(int T, int B, const float* reward_dev, const float* value_dev, const float* final_value_dev,
           const uint8_t* truncated_dev, float gamma, float lambda, float* advantage_out, float* returns_out, void* stream);

/* The same for agents that share their env's reward (wg_rollout_multi's buffers): value / final_value / advantage / returns
 * are [T, B, A], reward / truncated [T, B]; agent row (b, a) runs the recurrence above with reward[t, b] and truncated[t, b].
 * A = 1 is wg_gae bit for bit.  The update is wg_ppo_update on the T * B * A agent rows: independent PPO with shared
 * parameters, each agent's critic on its own observation.  (A centralised critic has ONE value per env: wg_gae on [T, B],
 * then wg_ppo_update_shared.)                                                                                       */
int wg_gae_shared(int T, int B, int A, const float* reward_dev, const float* value_dev, const float* final_value_dev,
                  const uint8_t* truncated_dev, float gamma, float lambda, float* advantage_out, float* returns_out, void* stream);

/* The optimiser of `p` (curriculum.py:544-560: PPO(...) owns torch.optim.Adam): Adam's moments and step count, the scratch
 * of the gradient kernel.  `p` must outlive it.  WG_ERR_INVALID: a policy without a critic or without log_std.     */
int wg_ppo_create(wg_policy p, wg_ppo* out);
int wg_ppo_destroy(wg_ppo o);

/* Checkpoint / resume (curriculum.py:544-560 saves and reloads models between stages): Adam's m then v as ONE host vector
 * of n = 2 * wg_policy_n_params floats, and the step count.  Synchronises the device.                              */
int wg_ppo_get_state(wg_ppo o, float* mv_host, size_t n, uint64_t* step);
int wg_ppo_set_state(wg_ppo o, const float* mv_host, size_t n, uint64_t step);

/* A rollout flattened to n_rows = T * B rows (device pointers; wg_rollout's obs[0..T-1], raw, logp and wg_gae's outputs). */
typedef struct wg_ppo_batch {
    const float* obs;        /* [n_rows, n_in]  */
    const float* raw;        /* [n_rows, n_out] the unclipped actions the buffer stores */
    const float* logp;       /* [n_rows]        log-probability at collection time      */
    const float* advantage;  /* [n_rows]        */
    const float* returns;    /* [n_rows]        */
    int64_t n_rows;
} wg_ppo_batch;

typedef struct wg_ppo_hyper {      /* SB3's PPO arguments of the same names (longer_steps_example.py:212-231) */
    float clip_range, vf_coef, ent_coef;
    int32_t normalize_advantage;   /* ignored for a minibatch of one row, as in SB3 */
} wg_ppo_hyper;

typedef struct wg_ppo_stats {      /* means over the minibatch: what SB3 logs as train/... */
    float pi_loss, v_loss, entropy, approx_kl, clip_fraction, loss, adv_mean, adv_std;
} wg_ppo_stats;

/* One minibatch of SB3's PPO.train (longer_steps_example.py:232-240), loss and gradient only: rows index_dev[0 .. n-1] of
 * the batch (int32, device; entries outside [0, n_rows) are skipped) or, with index_dev = NULL, rows first .. first + n - 1.
 *   logp = sum_j (-((raw_j - mean_j) / exp(log_std_j))^2 / 2 - log_std_j - log(2 pi) / 2),   ratio = exp(logp - logp_old),
 *   A^ = (A - mean_mb(A)) / (std_mb(A) + 1e-8) (unbiased std) with normalize_advantage, else A,
 *   L_pi = -min(ratio A^, clip(ratio, 1 - eps, 1 + eps) A^),  L_v = (returns - V)^2,  H = sum_j (1/2 + log(2 pi)/2 + log_std_j),
 *   loss = mean(L_pi) + vf_coef mean(L_v) - ent_coef mean(H),   approx_kl = mean((ratio - 1) - log ratio),
 *   clip_fraction = mean(|ratio - 1| > eps).
 * grad_out f32[wg_policy_n_params] = d loss / d params in the flat layout of wg_policy_set_params; stats_out (device, may be
 * NULL) the record above.  params_dev must be the vector the policy was last given (wg_policy_set_params / wg_ppo_apply):
 * the forward pass is k_policy's, so with unchanged parameters ratio = 1 to rounding.  A data-parallel trainer all-reduces
 * grad_out between this call and wg_ppo_apply.  WG_ERR_INVALID: null / out-of-range arguments; a SPLIT policy
 * (wg_policy_create_vf, n_in_vf != n_in) — its critic cannot read `obs`, whose rows have the actor's width: nothing is enqueued,
 * the message names both widths and wg_ppo_grad_shared.                                                               */
int wg_ppo_grad(wg_ppo o, const float* params_dev, const wg_ppo_batch* batch, const int32_t* index_dev, int64_t first, int n,
                const wg_ppo_hyper* hp, float* grad_out, wg_ppo_stats* stats_out, void* stream);

/* torch.nn.utils.clip_grad_norm_(max_grad_norm) + torch.optim.Adam.step (betas 0.9 / 0.999, eps 1e-5 as SB3's PPO sets it,
 * bias-corrected, no weight decay) on params_dev IN PLACE, then wg_policy_set_params(p, params_dev) in stream order:
 * wg_policy_act / wg_rollout enqueued afterwards see the new weights (longer_steps_example.py:232-240).            */
int wg_ppo_apply(wg_ppo o, float* params_dev, const float* grad_dev, float lr, float max_grad_norm, void* stream);

/* SB3's PPO.train for one rollout (longer_steps_example.py:232-240), enqueued by one call, no host synchronisation, no
 * allocation: n_mb = ceil(n_rows / batch_size) minibatches per epoch, the last one shorter when batch_size does not divide
 * n_rows (as SB3's RolloutBuffer.get yields it); perm_dev int32[n_epochs, n_rows] holds a permutation of 0 .. n_rows-1 per
 * epoch; stats_out (device, may be NULL) is wg_ppo_stats[n_epochs, n_mb].  Bit-identical to
 *     for e in 0 .. n_epochs-1:  for k in 0 .. n_mb-1:
 *         wg_ppo_grad(o, params_dev, batch, perm_dev + e * n_rows + k * batch_size, 0, min(batch_size, n_rows - k * batch_size),
 *                     hp, g, stats_out + e * n_mb + k);   wg_ppo_apply(o, params_dev, g, lr, max_grad_norm)
 * WG_ERR_INVALID: as wg_ppo_grad, a split policy included (nothing is enqueued; use wg_ppo_update_shared).                  */
int wg_ppo_update(wg_ppo o, float* params_dev, const wg_ppo_batch* batch, const int32_t* perm_dev, int n_epochs,
                  int batch_size, const wg_ppo_hyper* hp, float lr, float max_grad_norm, wg_ppo_stats* stats_out, void* stream);

/* A rollout of agents that share their env's critic (wg_rollout_multi's central mode): every minibatch entry is an AGENT row
 * and carries its env's state — multi-agent PPO as published (MAPPO).  Agent row id belongs to env row e = id / agents.     */
typedef struct wg_ppo_batch_shared {
    wg_ppo_batch rows;     /* obs [n_rows, n_in], raw, logp [n_rows]: AGENT rows;  advantage, returns: [n_rows / agents] ENV rows */
    const float* obs_vf;   /* [n_rows / agents, n_in_vf]  what the critic reads: the env rows' flat observation                   */
    int32_t agents;        /* >= 1, divides n_rows                                                                               */
} wg_ppo_batch_shared;

/* wg_ppo_grad on such a batch.  For minibatch entry id, e = id / agents: the actor term uses obs[id], raw[id], logp[id] and
 * A = advantage[e]; the advantage normalisation is the mean / unbiased std of advantage[id / agents] over the minibatch's entries;
 * L_v = (returns[e] - V(obs_vf[e]))^2, averaged over the minibatch's ENTRIES (an env row drawn through two of its agents counts
 * twice).  Everything else — index_dev / first / n in agent rows, the statistics record, the determinism contract — as
 * wg_ppo_grad, which is this call on {*batch, batch->obs, 1}: with agents = 1, n_in_vf = n_in and obs_vf = obs the two are
 * bit-identical (on an equal-width policy: a split one is only accepted here).  WG_ERR_INVALID also for agents < 1 or not
 * dividing n_rows, a null obs_vf.                                                                                     */
int wg_ppo_grad_shared(wg_ppo o, const float* params_dev, const wg_ppo_batch_shared* batch, const int32_t* index_dev, int64_t first,
                       int n, const wg_ppo_hyper* hp, float* grad_out, wg_ppo_stats* stats_out, void* stream);

/* wg_ppo_update on such a batch: perm_dev int32[n_epochs, n_rows] permutes AGENT rows, batch_size counts them.  Bit-identical to
 * wg_ppo_update's loop with wg_ppo_grad_shared in place of wg_ppo_grad; wg_ppo_update is this call on {*batch, batch->obs, 1}. */
int wg_ppo_update_shared(wg_ppo o, float* params_dev, const wg_ppo_batch_shared* batch, const int32_t* perm_dev, int n_epochs,
                         int batch_size, const wg_ppo_hyper* hp, float lr, float max_grad_norm, wg_ppo_stats* stats_out, void* stream);

/* A KL-ADAPTIVE LEARNING RATE on the device (the schedule of rsl_rl / rl_games, minibatch by minibatch): the rate lives in ONE
 * device float and follows the approx_kl each minibatch's reduce has just written, with no host round trip and no launch of its
 * own (the Adam kernel reads both words).  THE RULE, from the rule the caller gives (band and `down` computed once in float on
 * the host: kl_low = desired_kl / 2, kl_high = 2 * desired_kl, up = factor, down = 1 / factor; multiplications only afterwards):
 *     next(lr, kl):  kl > kl_high              -> max(lr_min, lr * down)
 *                    kl < kl_low and kl > 0    -> min(lr_max, lr * up)
 *                    else (inside the band, kl == 0, kl < 0, NaN) -> lr
 * While set on a handle, wg_ppo_update and wg_ppo_update_shared on it (and wg_pop_update for a member whose opts[m] it is) IGNORE
 * their lr argument and are bit-identical to wg_ppo_update's loop with
 *     lr = *lr_dev
 *     for e, k:  wg_ppo_grad(..., stats + e * n_mb + k)
 *                if (e, k) != (0, 0):  lr = next(lr, stats[e * n_mb + k].approx_kl)
 *                wg_ppo_apply(o, params_dev, g, lr, max_grad_norm)
 *     *lr_dev = lr                      (visible in stream order after the call)
 * The FIRST minibatch of an update never moves the rate: the parameters are still the rollout's there, ratio = 1 to rounding
 * (wg_ppo_grad), so the sign and size of its approx_kl are noise.  stats_out = NULL changes nothing (the handle reads its own
 * record).  Adam's step_size is float((double)lr / (1 - beta1^step)) formed in the kernel from the rate it read: the bits of
 * wg_ppo_apply with that lr.  wg_ppo_grad, wg_ppo_apply and wg_bc_* are unaffected (apply takes its argument; a supervised
 * loss has no KL).
 * lr_dev: one caller-owned device float on the handle's device — the starting rate, updated in place, and it must outlive the
 * setting.  rule = NULL together with lr_dev = NULL turns the rule off again.  Reads *lr_dev once (synchronises the device).
 * WG_ERR_INVALID, naming the argument: one of rule / lr_dev null; desired_kl not > 0 or not finite; factor < 1 or not finite;
 * lr_min not > 0; lr_min > lr_max; lr_dev not memory of the handle's device; a starting rate outside [lr_min, lr_max].        */
typedef struct wg_kl_lr {
    float desired_kl;      /* the KL the rate steers toward: it stays while desired_kl / 2 <= approx_kl <= 2 desired_kl */
    float factor;          /* >= 1: the rate is multiplied by it below the band, by 1 / factor above (rsl_rl: 1.5)      */
    float lr_min, lr_max;  /* the clamp (rsl_rl: 1e-5, 1e-2)                                                            */
} wg_kl_lr;
int wg_ppo_set_kl_lr(wg_ppo o, const wg_kl_lr* rule, float* lr_dev);

/* -----------------------------------------------------------------------------------------------------------------
 * Behaviour cloning: a SUPERVISED loss on the same handle — the optimiser's Adam state, its scratch and wg_ppo_apply are the
 * ones above, and k_bc_grad is k_ppo_grad's forward and backward with another loss head (windgym_amd/csrc/wg_ppo.hip).  The
 * expert's actions come from wg_expert_labels below.
 * --------------------------------------------------------------------------------------------------------------- */
#define WG_BC_MSE 0
#define WG_BC_NLL 1

typedef struct wg_bc_batch {
    const float* obs;        /* [n_rows, n_in]  */
    const float* target;     /* [n_rows, n_out] the expert's actions */
    const float* returns;    /* [n_rows], or NULL: no critic term    */
    int64_t n_rows;
} wg_bc_batch;

typedef struct wg_bc_hyper {
    int32_t loss;            /* WG_BC_MSE, WG_BC_NLL */
    float ent_coef, vf_coef; /* ent_coef: WG_BC_NLL only; vf_coef: only with returns */
} wg_bc_hyper;

typedef struct wg_bc_stats {       /* means over the minibatch; mse, nll, entropy and mean_abs_err whichever loss was chosen */
    float loss, mse, nll, entropy, v_loss, mean_abs_err, reserved[2];
} wg_bc_stats;

/* One minibatch, loss and gradient only; the rows are chosen as wg_ppo_grad chooses them (index_dev[0 .. n-1] with entries
 * outside [0, n_rows) skipped, or first .. first + n - 1; every mean divides by n).  With mean = the actor's output, logp and H
 * as wg_ppo_grad defines them (`target` in place of `raw`):
 *   mse = mean_rows((1 / n_out) sum_j (mean_j - target_j)^2),   nll = -mean_rows(logp(target)),   entropy = H,
 *   mean_abs_err = mean_rows((1 / n_out) sum_j |mean_j - target_j|),   v_loss = mean_rows((returns - V)^2) (0 without returns),
 *   WG_BC_MSE: loss = mse                       — the gradient of every log_std entry is exactly 0.0f;
 *   WG_BC_NLL: loss = nll - ent_coef * H;
 *   with returns both add vf_coef * v_loss; without, every critic entry of grad_out is exactly 0.0f (the critic's workgroups are
 *   not launched) and v_loss is 0 — also on a handle whose scratch an earlier wg_ppo_grad or wg_bc_grad filled.
 * Deterministic as wg_ppo_grad.  WG_ERR_INVALID: null / out-of-range arguments, an unknown loss, a split policy
 * (wg_policy_create_vf) — nothing is enqueued.                                                                          */
int wg_bc_grad(wg_ppo o, const float* params_dev, const wg_bc_batch* batch, const int32_t* index_dev, int64_t first, int n,
               const wg_bc_hyper* hp, float* grad_out, wg_bc_stats* stats_out, void* stream);

/* n_epochs passes over the batch in minibatches of batch_size rows (the last one shorter), as wg_ppo_update walks them:
 * perm_dev int32[n_epochs, n_rows], stats_out (device, may be NULL) wg_bc_stats[n_epochs, n_mb], n_mb = ceil(n_rows / batch_size).
 * Bit-identical to
 *     for e in 0 .. n_epochs-1:  for k in 0 .. n_mb-1:
 *         wg_bc_grad(o, params_dev, batch, perm_dev + e * n_rows + k * batch_size, 0, min(batch_size, n_rows - k * batch_size),
 *                    hp, g, stats_out + e * n_mb + k);   wg_ppo_apply(o, params_dev, g, lr, max_grad_norm)                      */
int wg_bc_update(wg_ppo o, float* params_dev, const wg_bc_batch* batch, const int32_t* perm_dev, int n_epochs, int batch_size,
                 const wg_bc_hyper* hp, float lr, float max_grad_norm, wg_bc_stats* stats_out, void* stream);

/* -----------------------------------------------------------------------------------------------------------------
 * Populations: P policies of ONE architecture collected and trained in the kernel launches of one (seeds of a result,
 * a sweep of gamma / learning rate / ent_coef: longer_steps_example.py + submit.sh run such sweeps as job arrays).
 * A population is P existing handles plus a small object that lets the kernels find them; the members stay ordinary
 * wg_policy / wg_ppo handles (wg_policy_act, wg_policy_set_params, wg_ppo_get_state ... work on a member as before).
 * Member m owns rows [m * Bm, (m + 1) * Bm) of every [.., B, ..] buffer, Bm = B / P.  CONTRACT: every entry below is
 * bit-identical, per member, to the loop of single-policy calls its comment names — a member's results depend neither on
 * P, nor on its index m, nor on what the other members hold (no float atomics, every sum in the single call's order).
 * A population is used on ONE stream at a time (its device tables are rewritten in stream order by each call).
 * Out of scope: wg_rollout_multi (per-agent and central), members of differing architectures.
 * --------------------------------------------------------------------------------------------------------------- */
#define WG_POP_MAX 16
typedef struct wg_pop_s* wg_pop;

/* members[0 .. P-1]: policies of ONE architecture (equal wg_policy_desc) on one device; opts[m] = the wg_ppo of members[m],
 * or opts = NULL for a population that only acts.  The handles must outlive the population.  WG_ERR_INVALID (the message
 * names the member): P outside 1 .. WG_POP_MAX, differing architectures or devices, a member listed twice, an opts[m] that
 * is not members[m]'s, a split policy (wg_policy_create_vf with another critic width).                                */
int wg_pop_create(const wg_policy* members, const wg_ppo* opts, int P, wg_pop* out);
int wg_pop_destroy(wg_pop q);

/* ONE launch of the policy kernel for all members: bit-identical to, for m in 0 .. P-1 with Bm = n_rows / P,
 *     wg_policy_act(members[m], Bm, obs_dev + m * Bm * n_in, deterministic, seeds[m], counter, row_offsets[m],
 *                   action_dev + m * Bm * n_out, raw_dev + m * Bm * n_out, logp_dev + m * Bm, value_dev + m * Bm, stream)
 * (null outputs are skipped for every member; row_offsets = NULL: all 0; seeds may be NULL when no actor output is wanted).
 * WG_ERR_INVALID, nothing enqueued: P does not divide n_rows; what wg_policy_act refuses.                               */
int wg_pop_act(wg_pop q, int n_rows, const float* obs_dev, int deterministic, const uint64_t* seeds, uint64_t counter,
               const uint64_t* row_offsets, float* action_dev, float* raw_dev, float* logp_dev, float* value_dev, void* stream);

/* wg_rollout with the population in the policy's place: the same buffers [T (+ 1), B, ..], member m on the envs (columns)
 * [m * Bm, (m + 1) * Bm).  Bit-identical (buffers and handle state) to wg_rollout's documented loop with each wg_policy_act
 * replaced by the P calls above (noise key of member m: seeds[m], counter0 + t, row_offsets[m] + its env's index in the
 * member) — still one launch of the policy kernel per step.  WG_ERR_INVALID: P does not divide the handle's n_envs; what
 * wg_rollout refuses.                                                                                                     */
int wg_pop_rollout(wg_handle h, wg_pop q, int n_steps, int deterministic, const uint64_t* seeds, uint64_t counter0,
                   const uint64_t* row_offsets, const wg_rollout_bufs* bufs, void* stream);

/* wg_gae on [T, B] with column b's member m = b / (B / P) choosing gamma[m] / lambda[m] (host arrays [P]): bit-identical to
 * wg_gae on the member's columns; with equal values it is wg_gae bit for bit.  WG_ERR_INVALID: P outside 1 .. WG_POP_MAX or
 * not dividing B.                                                                                                         */
int wg_gae_pop(int T, int B, int P, const float* reward_dev, const float* value_dev, const float* final_value_dev,
               const uint8_t* truncated_dev, const float* gamma, const float* lambda, float* advantage_out, float* returns_out,
               void* stream);

/* SB3's PPO.train for every member on ONE batch (wg_rollout's buffers flattened to n_rows = T * B rows), in the launches of
 * one wg_ppo_update: rows_m = n_rows / P rows per member, perm_dev int32[P, n_epochs, rows_m] holds per member and epoch a
 * permutation of ITS rows as GLOBAL row ids of the batch (row r of member m of a [T, B] rollout: (r / Bm) * B + m * Bm + r % Bm),
 * the same n_mb = ceil(rows_m / batch_size) minibatches for every member (the launches run in lockstep); hp, lr and
 * max_grad_norm are host arrays [P]; params_dev[m] (host array of device pointers) is the flat vector members[m] was last
 * given; stats_out (device, may be NULL) is wg_ppo_stats[P, n_epochs, n_mb].  Bit-identical, per member, to
 *     wg_ppo_update(opts[m], params_dev[m], <the member's rows as a contiguous batch>, <the same permutations as local row ids>,
 *                   n_epochs, batch_size, &hp[m], lr[m], max_grad_norm[m], stats_out + m * n_epochs * n_mb, stream)
 * and Adam's step count advances in every member's own wg_ppo.  WG_ERR_INVALID, nothing enqueued: a population created
 * without opts, P not dividing n_rows, what wg_ppo_update refuses (the message names the member).
 * With wg_ppo_set_kl_lr on the members' handles every member's rate is its own device word under its own rule (lr[m] is ignored)
 * and the contract above holds with that rule set on the single-policy call, whatever P, m and the other members' rules; the
 * launches run in lockstep, so EVERY member is set or none: anything else (or one lr_dev given to two members) is WG_ERR_INVALID
 * naming the member, nothing enqueued.                                                                                     */
int wg_pop_update(wg_pop q, float* const* params_dev, const wg_ppo_batch* batch, const int32_t* perm_dev, int n_epochs,
                  int batch_size, const wg_ppo_hyper* hp, const float* lr, const float* max_grad_norm, wg_ppo_stats* stats_out,
                  void* stream);

/* -----------------------------------------------------------------------------------------------------------------
 * Yaw-curriculum reward shaping: the reference's CurriculumWrapper + CurriculumCallback (examples/curriculum.py:335-429) as a
 * POST-PASS over a rollout's buffers, like wg_gae — the policy never reads the reward while it collects, so nothing is added
 * to the step kernels or to wg_rollout (windgym_amd/csrc/wg_curriculum.hip).  Per env, with state that lives in the
 * wg_curriculum and, as in the wrapper, is never cleared (not by an episode's end either; MODEL.md lists the quirks):
 *     y = the yaws the agent farm held after the step's actuation, BEFORE a same-step autoreset;  g = the target yaws of the
 *     episode the step belongs to (Serial-Refine optimum of its wind: wg_steady_optimize);  r = the env's reward;  n = steps
 *     shaped so far;
 *     d = mean_i |y_i - g_i|;  sim = 1 / (1 + d);  pen = 0
 *     if n >= 1:  c_i = |y_i - yprev_i|;  pen += 0.3 * mean_i(c_i) / yaw_max;  cum += sum_i c_i
 *                 if n >= 2:  osc += sum_i |sign(c_i) - sprev_i|;  pen += 0.2 * osc / ((n - 1) * N)
 *                 if n >= 5:  pen += 0.1 * (cum / N) / yaw_max
 *                 sprev_i = sign(c_i)
 *     yprev = y;  n += 1
 *     cur = (1 - w) * (sim - pen / 600) + w * r;   out = last = momentum * last + (1 - momentum) * cur
 * fp64 arithmetic and state (osc and n are integers), sums over the turbines in index order, no atomics; the fp32 outputs are
 * rounded once at the store.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct wg_curriculum_s* wg_curriculum;

/* Per-env state for the B envs x N turbines of `h`, on its device, all zero (yprev, sprev, n, osc, cum, last and the running
 * targets g).  The batch geometry and the yaw actuation (yaw_min / yaw_max / yaw_step, action method) are copied from `h`:
 * the curriculum does not need the handle afterwards.                                                                  */
int wg_curriculum_create(wg_handle h, wg_curriculum* out);
int wg_curriculum_destroy(wg_curriculum c);

/* Checkpoint: the whole state as one host blob (call with host == NULL for the size) behind a header (magic, B, N);
 * wg_curriculum_set_state refuses a blob of another geometry.  Both synchronise the device.  wg_curriculum_get_state is also
 * where an ep_row_dev entry >= C met by an earlier wg_curriculum_shape is reported (that call is asynchronous and cannot
 * return what only the device saw: the kernel skips such an entry and latches it): WG_ERR_INVALID once, naming ep_row_dev. */
int wg_curriculum_get_state(wg_curriculum c, void* host, size_t* size);
int wg_curriculum_set_state(wg_curriculum c, const void* host, size_t size);

/* The running targets g of every env (CurriculumWrapper.reset for the whole batch): yaw_dev f64[B, N], copied in stream order. */
int wg_curriculum_set_targets(wg_curriculum c, const double* yaw_dev /* [B, N] */, void* stream);

/* Shape T steps of a rollout: ONE launch of k_curriculum (one thread per env walks its T steps), asynchronous on `stream`,
 * allocates nothing.  Shaping T steps in one call is bit-identical to shaping them in two.
 * WG_INFO_YAW_AGENT recorded after a truncating step is already the next episode's initial yaw, so the kernel restates the
 * env's fp32 actuation (WindFarmEnv._adjust_yaws, both action methods): y_t = adjust(prev, action_t) with prev = yaw0 for
 * t = 0 and yaw_after[t - 1] afterwards — which also carries a new episode's initial yaws.  On the step that truncates the
 * reward uses the old episode's g; where truncated_dev[t, b] != 0 and ep_row_dev[t, b] >= 0, g becomes row ep_row_dev[t, b] of
 * ep_target_dev from step t + 1 on (ep_row_dev is read only there; -1 keeps the target).  weight_dev[t] is w of step t.
 * WG_ERR_INVALID, nothing enqueued, the message naming the argument: a null required buffer (ep_target_dev may be NULL with
 * C == 0), T < 0, C < 0, momentum outside [0, 1), a buffer that is not device memory of the curriculum's device (the device of
 * the handle it was created on).  T == 0 does nothing.                                                                  */
int wg_curriculum_shape(wg_curriculum c, int T,
        const float* yaw0_dev,          /* [B, N]    yaws before the first step                              */
        const float* actions_dev,       /* [T, B, N] what wg_step received                                   */
        const float* yaw_after_dev,     /* [T, B, N] WG_INFO_YAW_AGENT recorded per step (AFTER an autoreset) */
        const uint8_t* truncated_dev,   /* [T, B]                                                            */
        const int32_t* ep_row_dev,      /* [T, B]    -1, or the row of ep_target that applies from step t + 1 */
        const double* ep_target_dev,    /* [C, N]                                                            */
        int C,
        const double* weight_dev,       /* [T]                                                               */
        double momentum,
        const float* reward_dev,        /* [T, B]                                                            */
        float* shaped_out,              /* [T, B]    may alias reward_dev                                    */
        float* yaw_diff_out,            /* [T, B]    or NULL: d of every step                                */
        float* yaw_out,                 /* [T, B, N] or NULL: y of every step                                */
        void* stream);

/* The expert's actions for a rollout of T steps on `h` (behaviour cloning from the yaw optimiser; wg_bc_update fits a policy to
 * them): ONE launch of k_expert_labels, one thread per env walking its T steps, asynchronous on `stream`, allocates nothing.
 * For step t, env b, turbine i:  prev = yaw0 for t = 0, else yaw_after[t - 1] — the yaw the observation of step t belongs to, a
 * new episode's initial yaw after a reset;  g = the env's running target in targets_dev, which becomes row ep_row_dev[t, b] of
 * ep_target_dev AFTER step t where truncated_dev[t, b] != 0 and that entry is >= 0 (k_curriculum's order).  The label is the
 * action that the env's actuation rule (yaw_min / yaw_max / yaw_step and the action method of `h`, as floats widened to double)
 * turns into the largest move towards g, computed in double and rounded once:
 *     WG_ACT_WIND:  a = (g - yaw_min) / (yaw_max - yaw_min) * 2 - 1        WG_ACT_YAW:  a = clamp((g - prev) / yaw_step, -1, 1)
 * yaw_diff_out[t, b] = (sum_i |prev_i - g_i|, in index order, in double) / N.  targets_dev is read and updated in place: after the
 * call it is what the next rollout starts from.  An ep_row_dev entry >= C is skipped and latched in err_dev (int32[4], device,
 * zeroed by the caller once; may be NULL: not latched), as wg_curriculum_shape latches it: wg_expert_labels_check synchronises
 * the device and returns WG_ERR_INVALID once, naming ep_row_dev, t, b and the entry.  WG_ERR_INVALID, nothing enqueued: a null
 * required buffer (ep_target_dev may be NULL with C == 0), T < 0, C < 0, a buffer off the handle's device.  T == 0 does nothing. */
int wg_expert_labels(wg_handle h, int T,
        const float* yaw0_dev,          /* [B, N]                                                            */
        const float* yaw_after_dev,     /* [T, B, N] WG_INFO_YAW_AGENT recorded per step (AFTER an autoreset) */
        const uint8_t* truncated_dev,   /* [T, B]                                                            */
        const int32_t* ep_row_dev,      /* [T, B]    -1, or the row of ep_target that applies from step t + 1 */
        const double* ep_target_dev,    /* [C, N]                                                            */
        int C,
        double* targets_dev,            /* [B, N]    the running targets, in and out                         */
        float* labels_out,              /* [T, B, N]                                                         */
        float* yaw_diff_out,            /* [T, B]    or NULL                                                 */
        int32_t* err_dev,               /* [4]       or NULL                                                 */
        void* stream);
int wg_expert_labels_check(wg_handle h, int32_t* err_dev);

/* -----------------------------------------------------------------------------------------------------------------
 * Yaw table: the Serial-Refine optimiser's yaws on a grid of wind conditions, resident on the device, looked up by the NEAREST
 * node (windgym_amd/csrc/wg_yaw_table.hip; the node rule is stated once, in windgym_amd/csrc/wg_yaw_table.h).  Three axes of
 * float64 nodes, each strictly ascending, in the order ti (slowest), ws, wd (fastest); C = n_ti * n_ws * n_wd rows of N yaws
 * (degrees).  For one axis a_0 < ... < a_{n-1} and a value x, in double:
 *     i = the number of midpoints m_k = (a_k + a_{k+1}) / 2, k = 0 .. n-2, with m_k < x
 * (a tie goes to the lower node, x outside the axis to the end node);  row = (i_ti * n_ws + i_ws) * n_wd + i_wd;  a wind with a
 * non-finite component has row -1.  wrap_wd != 0 (the caller's statement that wd covers the full circle): x is first reduced by
 *     r = fmod(x - a_0, 360);  if (r < 0) r += 360;  x = a_0 + r
 * and a virtual node a_0 + 360 maps to index 0.  Nothing is interpolated: the optimum is an argmax over discrete candidates and
 * is not continuous in the wind.  A wind is three doubles (ws, wd, ti), the layout of WG_INFO_WIND_F64.  No kernel here sums,
 * uses atomics or allocates; every value is a fixed fp64 expression rounded at most once.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct wg_yaw_table_s* wg_yaw_table;

/* The table on `device`: the axes are HOST arrays, yaw f64[C, N] is a host array or (on_device != 0) memory of `device`; both are
 * copied into ONE allocation, which is all the table ever allocates.  Synchronises the device.  WG_ERR_INVALID, the message naming
 * the argument: out / an axis / yaw null, an axis empty, not finite or not strictly ascending, wrap_wd with wd[n_wd - 1] - wd[0]
 * >= 360, N < 1, yaw (on_device) not memory of `device`.  WG_ERR_UNSUPPORTED: more than 1024 nodes on the three axes together
 * (what a workgroup stages in LDS), more than 2^31 entries.                                                              */
int wg_yaw_table_create(int device, const double* ti, int n_ti, const double* ws, int n_ws, const double* wd, int n_wd,
                        int wrap_wd, int N, const double* yaw, int on_device, wg_yaw_table* out);
int wg_yaw_table_destroy(wg_yaw_table tab);

/* The row of each of n winds: ONE launch of k_yaw_table_rows (one thread per wind), asynchronous on `stream`.  Reads wind_dev
 * f64[n, 3] and mask_dev u8[n] (may be NULL: every wind is looked up); writes rows_out i32[n]: the row, or -1 where the mask is 0
 * or the wind is not finite.  With the recorded WG_INFO_WIND_F64 and truncated of a rollout (n = T * B) rows_out is the ep_row_dev
 * of wg_curriculum_shape / wg_expert_labels, whose ep_target_dev is then the table's yaw and whose C its row count.
 * WG_ERR_INVALID, nothing enqueued: tab / wind_dev / rows_out null, n < 0, a buffer that is not memory of the table's device.
 * n == 0 does nothing.                                                                                                  */
int wg_yaw_table_rows(wg_yaw_table tab, int n, const double* wind_dev, const uint8_t* mask_dev, int32_t* rows_out, void* stream);

/* The yaws of each of n winds: ONE launch of k_yaw_table_targets (one thread per (wind, turbine)), asynchronous on `stream`.
 * Reads wind_dev f64[n, 3]; writes targets_out f64[n, N] = the table's row of every wind; the output row of a wind without a row
 * (-1) is left as it was.  WG_ERR_INVALID, nothing enqueued: tab / wind_dev / targets_out null, n < 0, a buffer that is not memory
 * of the table's device; WG_ERR_UNSUPPORTED: n * N > 2^31.  n == 0 does nothing.                                           */
int wg_yaw_table_targets(wg_yaw_table tab, int n, const double* wind_dev, double* targets_out, void* stream);

/* The table as a scripted agent: ONE launch of k_yaw_table_act (one thread per (env, turbine)), asynchronous on `stream`, no
 * state.  Reads, on the device, every env's current wind and the agent farm's current yaws (what WG_INFO_WIND_F64 and
 * WG_INFO_YAW_AGENT report) and writes action_out f32[B, N]: with g = the table's yaw of the wind's row and prev = the current
 * yaw, the action of wg_expert_labels, in double, rounded once:
 *     WG_ACT_WIND:  a = (g - yaw_min) / (yaw_max - yaw_min) * 2 - 1        WG_ACT_YAW:  a = clamp((g - prev) / yaw_step, -1, 1)
 * (a wind without a row, which no env samples: a = 0).  The lookup is repeated from the env's current wind on every call, so a
 * same-step autoreset needs no bookkeeping.  WG_ERR_INVALID, nothing enqueued: h / tab / action_out null, tab created for another
 * N than the handle's n_turb or on another device.                                                                       */
int wg_yaw_table_act(wg_handle h, wg_yaw_table tab, float* action_out, void* stream);

/* wg_rollout with the table in the policy's place: per step ONE launch of k_yaw_table_act -> actions[t], then the step and the
 * info recordings of wg_rollout.  Buffers and the handle's state afterwards are BIT-IDENTICAL to
 *     for t in 0 .. T-1:
 *         wg_yaw_table_act(h, tab, actions[t])
 *         wg_step(h, actions[t], obs[t+1], reward[t], truncated[t], final_obs[t])
 *         wg_get_info(h, info_fields[i], info_out[i] + t * <size of the field>)       for every i
 * WG_ERR_INVALID, nothing enqueued: a null argument, what wg_yaw_table_act refuses of tab, n_steps < 0, obs / actions / reward /
 * truncated missing, raw / logp / value / final_value not NULL (a table samples nothing and has no critic), bad info arguments. */
int wg_rollout_table(wg_handle h, wg_yaw_table tab, int n_steps, const wg_rollout_bufs* bufs, void* stream);

/* -----------------------------------------------------------------------------------------------------------------
 * VecNormalize: running observation / return statistics for PPO, restated from stable-baselines3 2.x
 * (common/vec_env/vec_normalize.py, common/running_mean_std.py; windgym_amd/csrc/wg_norm.hip).
 *   RunningMeanStd(shape): mean = 0, var = 1, count = 1e-4 (float64).  update(batch [n, ...]):
 *       bm = mean(batch, 0);  bv = var(batch, 0) (population variance about bm);  delta = bm - mean;  tot = count + n
 *       mean += delta * n / tot;  var = (var * count + bv * n + delta^2 * count * n / tot) / tot;  count = tot
 *   A wg_norm keeps obs_rms = RunningMeanStd((O,)), ret_rms = RunningMeanStd(()) and returns f64[B] = 0.
 *       normalize_obs(x)    = clip((x - obs_rms.mean) / sqrt(obs_rms.var + epsilon), +-clip_obs)        (identity: norm_obs == 0)
 *       normalize_reward(r) = clip(r / sqrt(ret_rms.var + epsilon), +-clip_reward)                      (identity: norm_reward == 0)
 *   One step of the wrapper, in this order (done = truncated: this env never terminates):
 *       1  obs, r, done = venv.step(a)              (obs: after an autoreset the NEW episode's first observation)
 *       2  if training and norm_obs: obs_rms.update(obs)
 *       3  obs_n = normalize_obs(obs)
 *       4  if training: returns = returns * gamma + r;  ret_rms.update(returns)
 *       5  r_n = normalize_reward(r)
 *       6  the terminal (final) rows = normalize_obs(.) with the statistics as they now stand; they never enter an update
 *       7  returns[done] = 0
 *   reset(): returns = 0; if training and norm_obs: obs_rms.update(obs); normalize_obs(obs).
 * Arithmetic: statistics and returns are float64; batch moments are computed in float64 from the float32 rows, the mean first,
 * then the squares about it; every sum has an order fixed by (n_rows, O) alone (no float atomics); a normalised value is
 * computed in float64, clipped and rounded to float32 once.  A wg_norm is used on one stream at a time.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct wg_norm_s* wg_norm;
typedef struct wg_norm_desc {
    int32_t n_obs, n_envs;         /* O and B                                                                         */
    int32_t norm_obs, norm_reward; /* 0: that half is the identity (and obs_rms is never updated when norm_obs == 0)  */
    float   clip_obs, clip_reward; /* > 0                                                                             */
    double  gamma, epsilon;        /* gamma in [0, 1]; epsilon in (0, 1)                                               */
} wg_norm_desc;

/* Fresh statistics on `device`, training on.  WG_ERR_INVALID: null argument, n_obs / n_envs < 1, a clip <= 0, gamma or
 * epsilon out of range.                                                                                               */
int wg_norm_create(const wg_norm_desc* d, int device, wg_norm* out);
int wg_norm_destroy(wg_norm n);

/* Checkpoint: one host blob (host == NULL: the size) = a header (magic, O, B, 0: int32) and then float64 obs mean [O], obs
 * var [O], obs count, ret mean, ret var, ret count, returns [B].  Both synchronise the device; wg_norm_set_state refuses a
 * blob of other widths (WG_ERR_INVALID).                                                                              */
int wg_norm_get_state(wg_norm n, void* host, size_t* size);
int wg_norm_set_state(wg_norm n, const void* host, size_t size);

/* training = 0 freezes both statistics (evaluation); normalisation goes on.  Takes effect for calls made afterwards.  */
int wg_norm_set_training(wg_norm n, int training);

/* returns = 0 for the envs whose byte of env_mask_host [B] is non-zero (NULL: all), in stream order: reset()'s step 2.  */
int wg_norm_reset_returns(wg_norm n, const uint8_t* env_mask_host /* NULL: all */, void* stream);

/* The observation half of one step (rules 2, 3 and 6): if training && norm_obs, obs_rms.update(the n_rows rows of obs_dev); then
 * out = normalize_obs(obs) and extra_out = normalize_obs(extra) (extra_dev / extra_out_dev may both be NULL: the final rows),
 * both with the statistics AFTER the update.  At most two launches (k_norm_part, k_norm_apply), asynchronous on `stream`, no
 * allocation, no host synchronisation.  Rows are [n_rows, O] float32.
 * WG_ERR_INVALID: null n / obs_dev / out_dev, one of extra_dev / extra_out_dev without the other, n_rows < 0, an update of more
 * than n_envs rows (a frozen wg_norm, or one with norm_obs == 0, takes any number).  n_rows == 0 does nothing.          */
int wg_norm_obs(wg_norm n, int n_rows, const float* obs_dev, float* out_dev, const float* extra_dev, float* extra_out_dev,
                void* stream);

/* The reward half of T steps as a post-pass over [T, B] (rules 4, 5 and 7 for t = 0 .. T-1 in order), like wg_gae: the policy
 * never reads the reward while it collects.  out_dev may alias reward_dev.  T steps in one call are bit-identical to T calls
 * of one step.  Asynchronous on `stream`; the fp64 scratch [T, B] is the wg_norm's and grows BEFORE anything is enqueued when T
 * exceeds every earlier call's (that call synchronises the device).  Equivalent loop:
 *     for t in 0 .. T-1:
 *         if training: returns = returns * gamma + reward[t];  ret_rms.update(returns)
 *         out[t] = normalize_reward(reward[t]);  returns[truncated[t] != 0] = 0
 * WG_ERR_INVALID: a null argument, T < 0.  T == 0 does nothing.                                                        */
int wg_norm_reward(wg_norm n, int T, const float* reward_dev, const uint8_t* truncated_dev, float* out_dev, void* stream);

/* wg_rollout with the policy reading NORMALISED rows whose statistics move inside the loop: buffers, the handle's state and the
 * wg_norm's state afterwards are BIT-IDENTICAL to wg_rollout's documented loop with obs[t] -> norm_obs[t] in the inputs of both
 * wg_policy_act calls (final_obs[t] -> norm_final_obs[t]) and, after each wg_step,
 *     wg_norm_obs(n, B, bufs->obs[t+1], norm_obs[t+1], bufs->final_obs[t], norm_final_obs[t])
 * norm_obs_dev [T+1, B, O] (slot 0 is INPUT: the normalised current observation), norm_final_obs_dev [T, B, O]; bufs->obs and
 * bufs->final_obs are required and hold the env's own rows.  With norm_obs == 0 the normalised buffers are copies and bufs is
 * filled bit for bit as wg_rollout fills it.  The reward is the env's: wg_norm_reward is a call of its own afterwards.
 * WG_ERR_INVALID: what wg_rollout refuses; a null wg_norm; one whose n_obs / n_envs are not the handle's obs_dim / n_envs or
 * that lives on another device; bufs->obs, bufs->final_obs, norm_obs_dev or norm_final_obs_dev missing.                  */
int wg_rollout_norm(wg_handle h, wg_policy p, wg_norm n, int n_steps, int deterministic, uint64_t seed, uint64_t counter0,
                    uint64_t row_offset, const wg_rollout_bufs* bufs, float* norm_obs_dev, float* norm_final_obs_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Recurrent policies: the LSTM front of sb3-contrib's MlpLstmPolicy (the reference's own trainer puts an nn.LSTM in front of its
 * actor and critic, examples/curriculum.py:109-146).  A wg_lstm is one (shared_lstm) or two (lstm_actor, lstm_critic) one-layer
 * LSTMs n_in -> hidden evaluated by ONE kernel (k_lstm, windgym_amd/csrc/wg_lstm.hip); the MLP behind it is an ordinary wg_policy
 * that maps hidden -> n_out with its critic on hidden.  The cell is torch.nn.LSTM's (gate order i, f, g, o):
 *     (h, c) <- (0, 0) for rows with episode_start != 0
 *     z = (b_ih + b_hh) + [W_ih | W_hh] (x ‖ h);  c' = sigmoid(z_f) c + sigmoid(z_i) tanh(z_g);  h' = sigmoid(z_o) tanh(c')
 * The episode-start mask is a SELECT: such a row does not depend on its incoming state at all, also where that state holds NaN
 * (sb3-contrib multiplies the state by 1 - episode_start; for finite states the two agree).  The two biases are added once, when
 * the parameters are packed, and the sum starts the k-ordered f32 accumulation over x then h.  Training through time is wg_lstm_ppo below, on what
 * wg_rollout_lstm records for it (the initial state, the episode starts).
 * Bounds (WG_ERR_UNSUPPORTED outside): n_in <= 2048, 1 <= hidden <= 256.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct wg_lstm_s* wg_lstm;
typedef struct wg_lstm_desc {
    int32_t n_in, hidden;
    int32_t n_nets;            /* 2: actor and critic LSTMs; 1: one LSTM whose h' both MLPs read (shared_lstm)       */
} wg_lstm_desc;
enum { WG_LSTM_ACTOR = 1, WG_LSTM_CRITIC = 2 };            /* bits of wg_lstm_step's net_mask                         */

int wg_lstm_create(const wg_lstm_desc* d, int device, wg_lstm* out);      /* all parameters 0 until wg_lstm_set_params */
int wg_lstm_destroy(wg_lstm l);
int wg_lstm_n_params(wg_lstm l, size_t* n);
/* All parameters as ONE flat f32 vector of wg_lstm_n_params floats: per net, the actor's first, weight_ih [4 hidden][n_in],
 * weight_hh [4 hidden][hidden], bias_ih [4 hidden], bias_hh [4 hidden] (torch.nn.LSTM's *_l0 tensors, rows in gate order
 * i, f, g, o).  Host (on_device = 0; must stay valid until the stream reaches the copy) or device pointer; stream-ordered copy +
 * repack into the kernel's layout, no synchronisation.                                                                */
int wg_lstm_set_params(wg_lstm l, const float* params, size_t n, int on_device, void* stream);

/* One step of the nets in net_mask (0 = all the handle has) on n_rows rows: x_dev f32[n_rows, n_in], episode_start_dev
 * u8[n_rows] or NULL (no row starts an episode), state_in_dev f32[n_nets][2][n_rows][hidden] (per net h then c; the planes of a
 * net that is masked out are neither read nor written) -> state_out_dev in the same layout and h_pi_dev / h_vf_dev
 * f32[n_rows, hidden], the new h of the actor's / the critic's LSTM.  state_out_dev may BE state_in_dev (in place), and may be
 * NULL: h' is computed and the new state discarded (what a bootstrap value of a final observation needs).  h_pi_dev / h_vf_dev
 * may be NULL.  fp32, bit-identical from run to run, and a row's result does not depend on n_rows, on the other rows or on
 * which nets the call evaluates.  One launch, asynchronous on `stream`, allocates and synchronises nothing.
 * WG_ERR_INVALID: a null x_dev / state_in_dev, n_rows < 0, a net_mask bit or an h output of a net the call does not evaluate. */
int wg_lstm_step(wg_lstm l, int n_rows, const float* x_dev, const uint8_t* episode_start_dev, const float* state_in_dev,
                 float* state_out_dev, float* h_pi_dev, float* h_vf_dev, int net_mask, void* stream);

/* The recurrent policy's wg_policy_act: `p` is an ordinary wg_policy that maps the LSTM's hidden size H -> n_out with its critic on H.
 * Two launches, bit-identical to
 *     wg_lstm_step(l, n_rows, x, episode_start, state_in, state_out, h_pi, h_vf, actor | (critic if value_dev and l has two nets))
 *     wg_policy_act(p, n_rows, h_pi, deterministic, seed, counter, row_offset, action, raw, logp, NULL)
 *     wg_policy_act(p, n_rows, h_vf, value only -> value_dev)            if wanted (a shared LSTM: h_vf = h_pi)
 * with h_pi = h_dev, h_vf = h_dev + n_rows * H: h_dev f32[2][n_rows][H] is the caller's scratch for the two h' row sets.  Without
 * value_dev the critic's LSTM is not evaluated and its planes of state_out_dev are not written.
 * WG_ERR_INVALID: what the two calls refuse; p's n_in or its critic's width != H; l and p on different devices.               */
int wg_lstm_act(wg_lstm l, wg_policy p, int n_rows, const float* x_dev, const uint8_t* episode_start_dev, const float* state_in_dev,
                float* state_out_dev, float* h_dev, int deterministic, uint64_t seed, uint64_t counter, uint64_t row_offset,
                float* action_dev, float* raw_dev, float* logp_dev, float* value_dev, void* stream);

/* Caller-owned device buffers of wg_rollout_lstm besides wg_rollout_bufs; B of the handle, H / nets of the wg_lstm. */
typedef struct wg_rollout_lstm_bufs {
    float*   state;          /* [nets][2][B][H]  in / out: the LSTM state the loop starts from and ends in                */
    float*   state0;         /* [nets][2][B][H]  or NULL: a copy of the incoming state (what a trainer unrolls from)      */
    uint8_t* episode_start;  /* [T+1, B]         slot 0 is INPUT; slot t+1 = truncated[t]                                  */
    float*   scratch;        /* [3][B][H]        the loop's h_pi, h_vf and the critic's h' on the final rows               */
} wg_rollout_lstm_bufs;

/* wg_rollout for a recurrent policy: `lstm` reads the observation rows, `p` is an ordinary wg_policy that maps H -> n_turb with
 * its critic on H.  Buffers, the handle's state and lstm_bufs->state afterwards are BIT-IDENTICAL to
 *     state0 = state                                                                        if wanted
 *     for t in 0 .. T-1:
 *         wg_lstm_step(lstm, B, obs[t], episode_start[t], state, state, h_pi, h_vf, all nets)       (a shared LSTM: h_vf = h_pi)
 *         wg_policy_act(p, B, h_pi, deterministic, seed, counter0 + t, row_offset, actions[t], raw[t], logp[t], NULL)
 *         wg_policy_act(p, B, h_vf, value only -> value[t])                                 if wanted
 *         wg_step(h, actions[t], obs[t+1], reward[t], truncated[t], final_obs[t])
 *         wg_get_info(h, info_fields[i], info_out[i] + t * <size of the field>)             for every i
 *         episode_start[t+1] = truncated[t]
 *         wg_lstm_step(lstm, B, final_obs[t], NULL, state, NULL, critic's net only -> h_fin)  \ if final_value
 *         wg_policy_act(p, B, h_fin, value only -> final_value[t])                            / is wanted
 * final_value[t] is sb3-contrib's bootstrap from the terminal LSTM state: the critic on (final_obs[t], the state after step t,
 * no episode start), that state left as it is.  For an env that was not truncated this is the arithmetic of step t+1's value.
 * A row's results do not depend on which launch computes them: the loop itself runs the final rows of step t-1 in front of step t.
 * WG_ERR_INVALID: what wg_rollout refuses, with p's n_in / its critic's width != lstm's hidden, lstm's n_in != the handle's
 * obs_dim, lstm on another device than the handle, a null lstm_bufs or one without state / episode_start / scratch.            */
int wg_rollout_lstm(wg_handle h, wg_lstm lstm, wg_policy p, int n_steps, int deterministic, uint64_t seed, uint64_t counter0,
                    uint64_t row_offset, const wg_rollout_bufs* bufs, const wg_rollout_lstm_bufs* lstm_bufs, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Training recurrent policies: sb3-contrib's RecurrentPPO.train for the wg_lstm + wg_policy pair above, by backpropagation through
 * time in HIP (windgym_amd/csrc/wg_lstm_ppo.hip).  fp32 throughout; every entry is asynchronous on `stream`, synchronises nothing
 * and is bit-identical from run to run (no atomics; every sum's order is fixed by T, the minibatch's size and the shapes).
 * ONE flat parameter vector of wg_lstm_ppo_n_params floats: the LSTM's (wg_lstm_set_params' order), then the MLP's
 * (wg_policy_set_params' order).
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct wg_lstm_ppo_s* wg_lstm_ppo;

/* One rollout as wg_rollout_lstm leaves it (device pointers), advantage / returns from wg_gae on [T, B]. */
typedef struct wg_lstm_ppo_batch {
    const float*   obs;            /* [T (+ 1), B, n_in]   the first T slots are read                                  */
    const float*   raw;            /* [T, B, n_out]                                                                   */
    const float*   logp;           /* [T, B]                                                                          */
    const float*   advantage;      /* [T, B]                                                                          */
    const float*   returns;        /* [T, B]                                                                          */
    const uint8_t* episode_start;  /* [T (+ 1), B]         the first T slots are read                                  */
    const float*   lstm_state0;    /* [nets][2][B][H]      the state the rollout began from                            */
    int32_t T, B;
} wg_lstm_ppo_batch;

/* The optimiser of the pair (l, p): Adam's moments and step count over the ONE flat vector, and the buffers of the sequence kernels
 * for minibatches of up to Bm_max envs x T_max steps (their size: wg_lstm_ppo.h).  l and p must outlive it.  WG_ERR_INVALID: null
 * arguments, p's n_in or its critic's width != l's hidden, a policy without critic or log_std, different devices, T_max or Bm_max
 * < 1.  WG_ERR_UNSUPPORTED, naming T_max and Bm_max: buffers beyond 16 GiB or more than 2^24 rows per minibatch.          */
int wg_lstm_ppo_create(wg_lstm l, wg_policy p, int T_max, int Bm_max, wg_lstm_ppo* out);
int wg_lstm_ppo_destroy(wg_lstm_ppo o);
int wg_lstm_ppo_n_params(wg_lstm_ppo o, size_t* n);

/* Adam's m then v as ONE host vector of 2 * wg_lstm_ppo_n_params floats, and the step count.  Synchronises the device. */
int wg_lstm_ppo_get_state(wg_lstm_ppo o, float* mv_host, size_t n, uint64_t* step);
int wg_lstm_ppo_set_state(wg_lstm_ppo o, const float* mv_host, size_t n, uint64_t step);

/* Loss and gradient of ONE minibatch of WHOLE env sequences: the envs envs_dev[0 .. n_envs-1] (int32, device; an entry outside
 * [0, B) is never dereferenced: the rule below) with all T steps of each, n = T * n_envs rows.
 *   an entry outside [0, B):  its T rows enter the heads as h = 0 with raw = logp = advantage = returns = 0; they count in n and in
 *     the advantage statistics like any row, and send no gradient into the LSTM.  The result does not depend on what the handle
 *     computed before;
 *   forward:  per env and net, (h, c) starts from lstm_state0[net][., env] — DATA, not a function of the parameters — and runs
 *     wg_lstm_step's cell over t = 0 .. T-1 with episode_start[t] as its SELECT (a fresh row reads zeros in place of its state,
 *     also where lstm_state0 holds NaN);
 *   loss:  wg_ppo_grad's, unchanged, on the n rows, the actor's MLP on the actor LSTM's h_t and the critic's on the critic LSTM's
 *     (the same rows when the LSTM is shared); normalize_advantage uses the mean and unbiased std of the minibatch's n rows;
 *   backward through time:  the gradient flows from (h_t, c_t) to (h_{t-1}, c_{t-1}) except across a step with episode_start[t] != 0,
 *     where it stops (the W_hh columns of such a step see h = 0); with a shared LSTM dh_t is the actor head's input gradient plus
 *     the critic head's, added in that order.
 * With whole-env minibatches this is sb3-contrib's sequence rule (sequences cut at episode starts, initial states from the rollout).
 * grad_out f32[wg_lstm_ppo_n_params] = d loss / d params; stats_out (device, may be NULL) wg_ppo_grad's record.  params_dev must be
 * the vector both handles were last given (wg_lstm_set_params + wg_policy_set_params, or wg_lstm_ppo_apply).
 * WG_ERR_INVALID: null arguments, T / B / n_envs < 1, clip_range < 0.  WG_ERR_UNSUPPORTED: T > T_max or n_envs > Bm_max.        */
int wg_lstm_ppo_grad(wg_lstm_ppo o, const float* params_dev, const wg_lstm_ppo_batch* batch, const int32_t* envs_dev, int n_envs,
                     const wg_ppo_hyper* hp, float* grad_out, wg_ppo_stats* stats_out, void* stream);

/* wg_ppo_apply's rule on the ONE flat vector: clipping by the global norm of the whole gradient, Adam (betas 0.9 / 0.999, eps 1e-5,
 * bias-corrected) on params_dev IN PLACE, then wg_lstm_set_params(l, params_dev) and wg_policy_set_params(p, params_dev + the
 * LSTM's count) in stream order.  WG_ERR_INVALID: null arguments, max_grad_norm <= 0.                                          */
int wg_lstm_ppo_apply(wg_lstm_ppo o, float* params_dev, const float* grad_dev, float lr, float max_grad_norm, void* stream);

/* All epochs and minibatches of one rollout, enqueued by one call with no host round trip: perm_dev int32[n_epochs, B] holds a
 * permutation of the envs 0 .. B-1 per epoch, n_mb = ceil(B / envs_per_batch) minibatches per epoch, the last one shorter when
 * envs_per_batch does not divide B; stats_out (device, may be NULL) is wg_ppo_stats[n_epochs, n_mb].  Bit-identical to
 *     for e in 0 .. n_epochs-1:  for k in 0 .. n_mb-1:
 *         wg_lstm_ppo_grad(o, params_dev, batch, perm_dev + e * B + k * envs_per_batch, min(envs_per_batch, B - k * envs_per_batch),
 *                          hp, g, stats_out + e * n_mb + k);   wg_lstm_ppo_apply(o, params_dev, g, lr, max_grad_norm)
 * lstm_state0 stays the rollout's: after the first minibatch it is stale, as in sb3-contrib.
 * WG_ERR_INVALID / WG_ERR_UNSUPPORTED: what the two calls refuse, n_epochs < 1.                                                 */
int wg_lstm_ppo_update(wg_lstm_ppo o, float* params_dev, const wg_lstm_ppo_batch* batch, const int32_t* perm_dev, int n_epochs,
                       int envs_per_batch, const wg_ppo_hyper* hp, float lr, float max_grad_norm, wg_ppo_stats* stats_out, void* stream);

/* wg_ppo_set_kl_lr (the rule, the loop, the skipped first minibatch and the refusals are stated there) for wg_lstm_ppo_update and,
 * per member, wg_lstm_pop_update: while set they ignore their lr argument and equal the loop above with the rate read from
 * *lr_dev and stepped by each minibatch's approx_kl before its wg_lstm_ppo_apply.  wg_lstm_ppo_grad, wg_lstm_ppo_apply and
 * wg_lstm_bc_* are unaffected.                                                                                                 */
int wg_lstm_ppo_set_kl_lr(wg_lstm_ppo o, const wg_kl_lr* rule, float* lr_dev);

/* ---------------------------------------------------------------------------------------------------------------
 * Behaviour cloning into a recurrent policy: the SUPERVISED loss of wg_bc_grad on the wg_lstm_ppo handle — its buffers, its Adam
 * state and wg_lstm_ppo_apply are the ones above, as wg_bc_* sits on wg_ppo; k_bc_grad_dh is k_bc_grad with the gradients of the h
 * rows, which the BPTT kernels above carry through time.  The expert's actions come from wg_expert_labels.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct wg_lstm_bc_batch {
    const float*   obs;            /* [T (+ 1), B, n_in]   the first T slots are read                                  */
    const float*   target;         /* [T, B, n_out]        the expert's actions                                        */
    const float*   returns;        /* [T, B] or NULL: the critic is left alone                                         */
    const uint8_t* episode_start;  /* [T (+ 1), B]         the first T slots are read                                  */
    const float*   lstm_state0;    /* [nets][2][B][H]      the state the rollout began from                            */
    int32_t T, B;
} wg_lstm_bc_batch;

/* Loss and gradient of ONE minibatch of WHOLE env sequences, n = T * n_envs rows: wg_lstm_ppo_grad's rule with wg_bc_grad's loss.
 *   forward and backward through time:  exactly wg_lstm_ppo_grad's — lstm_state0 is DATA, episode_start[t] is the cell's SELECT, and
 *     the gradient stops at a step with episode_start[t] != 0;
 *   loss:  exactly wg_bc_grad's over the n rows, the actor's MLP on the actor LSTM's h_t and the critic's on the critic LSTM's (the same
 *     rows when the LSTM is shared), `target` in place of `raw`:
 *       WG_BC_MSE: loss = mse                — the gradient of every log_std entry is exactly 0.0f;
 *       WG_BC_NLL: loss = nll - ent_coef * H;
 *       with returns both add vf_coef * v_loss, and with a shared LSTM dh_t is the actor head's input gradient plus the critic head's,
 *       in that order;
 *       without returns v_loss is 0 and the critic gets NO gradient: every critic entry of grad_out — the critic's MLP, and with two
 *       LSTMs the critic LSTM's whole block — is exactly +0.0f, with a shared LSTM dh_t is the actor head's term alone, and the
 *       critic's side of the kernels is not launched (with two LSTMs: half of the sequence work) — also on a handle whose scratch an
 *       earlier wg_lstm_ppo_grad or wg_lstm_bc_grad filled: nothing such a call left behind is read;
 *   an entry of envs_dev outside [0, B):  never dereferenced.  Its T rows reach the heads as h = 0 with target = returns = 0, count in
 *     n, and send nothing into the LSTM.  The rows of target / returns that no column of the minibatch names are not read.
 * grad_out f32[wg_lstm_ppo_n_params]; stats_out (device, may be NULL) wg_bc_grad's record.  Deterministic as wg_lstm_ppo_grad;
 * params_dev as there.  WG_ERR_INVALID: null arguments (the message names the batch pointer; only returns may be null), T / B /
 * n_envs < 1, a loss other than WG_BC_MSE / WG_BC_NLL, vf_coef or ent_coef < 0.  WG_ERR_UNSUPPORTED: T > T_max or n_envs > Bm_max. */
int wg_lstm_bc_grad(wg_lstm_ppo o, const float* params_dev, const wg_lstm_bc_batch* batch, const int32_t* envs_dev, int n_envs,
                    const wg_bc_hyper* hp, float* grad_out, wg_bc_stats* stats_out, void* stream);

/* All epochs and minibatches of one rollout, as wg_lstm_ppo_update walks them (perm_dev int32[n_epochs, B], n_mb = ceil(B /
 * envs_per_batch), the last minibatch shorter), enqueued by one call with no host round trip and no atomics; stats_out (device, may
 * be NULL) is wg_bc_stats[n_epochs, n_mb].  Bit-identical to
 *     for e in 0 .. n_epochs-1:  for k in 0 .. n_mb-1:
 *         wg_lstm_bc_grad(o, params_dev, batch, perm_dev + e * B + k * envs_per_batch, min(envs_per_batch, B - k * envs_per_batch),
 *                         hp, g, stats_out + e * n_mb + k);   wg_lstm_ppo_apply(o, params_dev, g, lr, max_grad_norm)
 * WG_ERR_INVALID / WG_ERR_UNSUPPORTED: what the two calls refuse, n_epochs < 1.                                                 */
int wg_lstm_bc_update(wg_lstm_ppo o, float* params_dev, const wg_lstm_bc_batch* batch, const int32_t* perm_dev, int n_epochs,
                      int envs_per_batch, const wg_bc_hyper* hp, float lr, float max_grad_norm, wg_bc_stats* stats_out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Populations of recurrent policies: P pairs (wg_lstm, wg_policy) of ONE architecture — the same n_in, hidden size, number of
 * LSTMs, heads and activation — collected and trained in the kernel launches of one (a seed sweep of small recurrent runs, each of
 * which leaves most of the device idle: one workgroup of the sequence kernels owns 32 envs for all T steps).  The population
 * contract above holds unchanged: member m owns rows / envs [m * Bm, (m + 1) * Bm), Bm = B / P, of every [.., B, ..] buffer, and
 * every entry below is bit-identical, per member, to the loop of single calls its comment names; a member's results depend neither
 * on P, nor on m, nor on what the other members hold (no float atomics, every sum in the single call's order).  The members stay
 * ordinary handles.  LSTM STATE of a population: [P][nets][2][Bm][H] — entry m is exactly the member's own wg_lstm_step state.
 * Used on ONE stream at a time.  Out of scope: wg_rollout_multi, members of differing architectures, HIP-graph capture.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct wg_lstm_pop_s* wg_lstm_pop;

/* lstms[m] / heads[m]: member m's pair, as wg_lstm_act takes it; opts[m] = the wg_lstm_ppo created for that pair, or opts = NULL
 * for a population that only acts.  The handles must outlive the population.  WG_ERR_INVALID (the message names the member): P
 * outside 1 .. WG_POP_MAX; a member with another n_in, hidden size, number of nets or head architecture than member 0; a head
 * that does not map the hidden size with its critic on the same width; another device; the same handle twice; an opts[m] made
 * for another pair.                                                                                                        */
int wg_lstm_pop_create(const wg_lstm* lstms, const wg_policy* heads, const wg_lstm_ppo* opts, int P, wg_lstm_pop* out);
int wg_lstm_pop_destroy(wg_lstm_pop q);

/* ONE launch of k_lstm and ONE of the policy kernel for all members: bit-identical to, for m in 0 .. P-1 with Bm = n_rows / P,
 *     wg_lstm_act(lstms[m], heads[m], Bm, x_dev + m * Bm * n_in, episode_start_dev + m * Bm, state_in_dev + m * S, state_out_dev + m * S,
 *                 <h rows>, deterministic, seeds[m], counter, row_offsets[m], action_dev + m * Bm * n_out, raw_dev + m * Bm * n_out,
 *                 logp_dev + m * Bm, value_dev + m * Bm, stream)                       S = nets * 2 * Bm * H floats
 * h_dev [2][n_rows][H] is scratch (member m's h rows are rows [m * Bm, (m + 1) * Bm) of each plane).  Null outputs are skipped for
 * every member; row_offsets = NULL: all 0.  WG_ERR_INVALID, nothing enqueued: P does not divide n_rows; seeds = NULL with an actor
 * output wanted; what wg_lstm_act refuses.                                                                                  */
int wg_lstm_pop_act(wg_lstm_pop q, int n_rows, const float* x_dev, const uint8_t* episode_start_dev, const float* state_in_dev,
                    float* state_out_dev, float* h_dev, int deterministic, const uint64_t* seeds, uint64_t counter,
                    const uint64_t* row_offsets, float* action_dev, float* raw_dev, float* logp_dev, float* value_dev, void* stream);

/* wg_rollout_lstm with the population in the pair's place: the same buffers [T (+ 1), B, ..], member m on the envs (columns)
 * [m * Bm, (m + 1) * Bm); lstm_bufs->state and ->state0 in the population's layout [P][nets][2][Bm][H].  Bit-identical (buffers, the
 * handle's state, the LSTM state) to wg_rollout_lstm's documented loop with each wg_lstm_step / wg_policy_act replaced by the P
 * calls on the members' rows (noise key of member m: seeds[m], counter0 + t, row_offsets[m] + its env's index in the member) —
 * per step the launches of wg_rollout_lstm, no more.  WG_ERR_INVALID: P does not divide the handle's n_envs; what
 * wg_rollout_lstm refuses.                                                                                                 */
int wg_lstm_pop_rollout(wg_handle h, wg_lstm_pop q, int n_steps, int deterministic, const uint64_t* seeds, uint64_t counter0,
                        const uint64_t* row_offsets, const wg_rollout_bufs* bufs, const wg_rollout_lstm_bufs* lstm_bufs, void* stream);

/* sb3-contrib's RecurrentPPO.train for every member on ONE rollout, in the launches of one wg_lstm_ppo_update.  `batch` is the
 * whole rollout [T, B] as wg_lstm_pop_rollout leaves it (lstm_state0 in the population's layout), advantage / returns from
 * wg_gae_pop; Bm = B / P envs per member; perm_dev int32[P, n_epochs, Bm] holds per member and epoch a permutation of ITS envs as
 * GLOBAL env ids (env e of member m: m * Bm + e); the same n_mb = ceil(Bm / envs_per_batch) minibatches for every member (the
 * launches run in lockstep); hp, lr and max_grad_norm are host arrays [P]; params_dev[m] (host array of device pointers) is the flat
 * vector member m's handles were last given; stats_out (device, may be NULL) is wg_ppo_stats[P, n_epochs, n_mb].  Bit-identical,
 * per member, to
 *     wg_lstm_ppo_update(opts[m], params_dev[m], <the member's columns as a contiguous batch [T, Bm], lstm_state0 = entry m>,
 *                        <the same permutations as local env ids>, n_epochs, envs_per_batch, &hp[m], lr[m], max_grad_norm[m],
 *                        stats_out + m * n_epochs * n_mb, stream)
 * and Adam's step count advances in every member's own wg_lstm_ppo.  An env id outside [0, B) is a column of zeros, as in
 * wg_lstm_ppo_grad; one inside [0, B) but outside the member's own envs is not checked (nothing is read out of bounds, but the rows are
 * another member's).  WG_ERR_INVALID / WG_ERR_UNSUPPORTED, nothing enqueued: a population created without opts, P not dividing B,
 * what wg_lstm_ppo_update refuses (T > T_max or envs_per_batch > Bm_max of a member's handle: the message names the member).
 * KL-adaptive rates (wg_lstm_ppo_set_kl_lr on the members' handles): as wg_pop_update states it — every member or none.         */
int wg_lstm_pop_update(wg_lstm_pop q, float* const* params_dev, const wg_lstm_ppo_batch* batch, const int32_t* perm_dev, int n_epochs,
                       int envs_per_batch, const wg_ppo_hyper* hp, const float* lr, const float* max_grad_norm, wg_ppo_stats* stats_out,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WINDGYM_HIP_H */

// nmpc_kernels.hip -- batched NMPC solve on MI355X (gfx950): PANOC inner iteration + L-BFGS +
// ALM/penalty outer loop, with the diff-drive rollout, stage/terminal costs, cross-track error and
// circle/ellipse soft-constraint penalties evaluated per step, entirely on device in f64.
//
// What is restated (paths relative to the reference repo):
//   cost / constraints   src/mpc/mpc_generator.py:66-171           (eval_psi)
//   solver               OpEn's PANOC + ALM that src/mpc/mpc_generator.py:173-193 generates and
//                        :206 calls; algorithm per SURVEY.md Appendix C  (solve kernel state machine)
// This file is original CDNA4 code; nothing here is translated from OpEn's Rust or CasADi's C.
#include "nmpc_device.h"
#include "../../include/nmpc_solver.h"

#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "nmpc_layout.h"
#include "nmpc_probe.h"
#include "nmpc_eval.h"
#include "nmpc_solve_common.h"
#include "nmpc_solve_hyb.h"
#include "nmpc_solve_hyb2.h"
#include "nmpc_rng.h"
#include "nmpc_geom.h"
#include "nmpc_loop.h"
#include "nmpc_plan.h"
#include "nmpc_order.h"
#include "nmpc_host.h"
#include "nmpc_launch.h"
static_assert(nmpc::LAUNCH_TEAM_WAVES == nmpc::TEAM_WAVES, "nmpc_launch.h: the waves of a team");

// =================================================================================================
// C ABI (include/nmpc_solver.h)
// =================================================================================================
using nmpc::DevBuf;
using nmpc::Event;
using nmpc::KArgs;
using nmpc::LdsMap;
using nmpc::PinBuf;

// Every instantiation of the solve kernels: host code names them here and nowhere else.  A row is picked once per handle (nmpc_new), and
// the name, the LDS attribute and the launch all go through it.  The rows' order is the kernels' order in the gfx950 code object (the
// first host reference decides it), and the headline kernel is sensitive to where it lies: keep it.
namespace nmpc {
struct SolveKernel {
    const char *name;      // nmpc_kernel_name: recorded profiles are keyed on it
    void (*fn)(KArgs);
    int P;                 // family: 20 = nmpc_solve_hyb_kernel, 40 = nmpc_solve_hyb2_kernel
    bool timed;            // Timed<>: the wall-clock test compiled in (nmpc_set_time_limits)
    int N, nobs, ndyn;     // the shape it is specialised for; N = 0: any
};
#define SOLVE_ROW(K, P, S) {#K "<" #S ">", K<S>, P, ShapeTimed<S>::value, S::N, S::NOBS, S::NDYN}
static const SolveKernel SOLVE_KERNELS[] = {
    SOLVE_ROW(nmpc_solve_hyb_kernel, 20, ShapeDefault),
    SOLVE_ROW(nmpc_solve_hyb_kernel, 20, ShapeNobs50),
    SOLVE_ROW(nmpc_solve_hyb_kernel, 20, ShapeAny),
    SOLVE_ROW(nmpc_solve_hyb_kernel, 20, Timed<ShapeDefault>),
    SOLVE_ROW(nmpc_solve_hyb_kernel, 20, Timed<ShapeNobs50>),
    SOLVE_ROW(nmpc_solve_hyb_kernel, 20, Timed<ShapeAny>),
    SOLVE_ROW(nmpc_solve_hyb2_kernel, 40, ShapeN40),
    SOLVE_ROW(nmpc_solve_hyb2_kernel, 40, ShapeAny),
    SOLVE_ROW(nmpc_solve_hyb2_kernel, 40, Timed<ShapeN40>),
    SOLVE_ROW(nmpc_solve_hyb2_kernel, 40, Timed<ShapeAny>),
};
#undef SOLVE_ROW
}  // namespace nmpc
using nmpc::SolveKernel;

// The three groups of resources a handle makes on first use, each all or none.
struct Staging {         // host path: buffers sized for max_batch, two pinned bounce buffers (pageable user memory <-> HBM at DMA speed)
    DevBuf<double> p, u, y0, c0, yout, psi, grad, F1, F2;
    DevBuf<nmpc_status> st;
    PinBuf pin[2];
    Event ev[2];
    bool ready = false;
};
// small batches through the host entry point (the reference's own call is B = 1, src/path_generator.py:385): ONE device arena
// [p | c0 | y0 | u | y_out | status] per instance block, one pinned mirror, one copy in (p .. u), one copy out (u .. status), two events kept
struct SmallArena {
    DevBuf<char> d;
    PinBuf h;
    Event ev[2];
    bool ready = false;
    void release() { *this = {}; }
};
struct Pools {           // instances that leave their wave: parked solver states, the pools' ring buffers and their counters
    DevBuf<double> park;
    DevBuf<int> pool;
    DevBuf<unsigned int> ctr;
    bool made() const { return park && pool && ctr; }
    void release() { *this = {}; }
};

struct nmpc_handle {
    nmpc_problem pb{};
    nmpc_opts op{};
    int device = 0;
    int max_batch = 0;
    bool alive = true;
    LdsMap map{};
    int P = 20;                // 20: three query points per wave, one stage per lane (N_hor <= 20); 40: three points, two stages per lane (20 < N_hor <= 40)
    const SolveKernel *kernel[2] = {nullptr, nullptr};   // the handle's rows of SOLVE_KERNELS: plain, Timed<>
    int grid_cap = 0;          // resident waves the launch is sized for
    double last_ms = 0.0;      // kernel time of the last host-path batch
    size_t team_lds = 0;       // solve kernels: dynamic LDS bytes of one workgroup (four slices + control block)
    size_t eval_lds = 0;       // eval kernels: dynamic LDS bytes of one wave (three instances, a slice each)
    DevBuf<unsigned int> d_queue;
    int park_min = 500, park_depth = 8;  // hybrid kernel: migrate instances after this many passes (0 = never) / pool depth limit
    int sched_mode = 1;            // step-aside scheduling (NMPC_SCHED=0 switches it off); long instances time-share beyond sched_theta x resident waves (NMPC_SCHED_THETA)
    double sched_theta = 0.0, sched_cold = 0.4;
    bool shape_any = false;        // experiments (NMPC_SHAPE=any): the run-time-shape kernel whatever the shape
    int team_owners_forced = 0;    // experiments (NMPC_TEAM_OWNERS): waves per workgroup that take instances, 0 = automatic
    bool team_help = true;         // experiments (NMPC_TEAM_HELP=0): helpers never asked
    int waves_per_cu = 0;          // experiments (NMPC_WAVES_PER_CU): resident waves per CU the launch is sized for, 0 = all that fit
    int dbg = 0;                   // experiments (NMPC_DEBUG_PRIO): KArgs.dbg
    double cull_radius = 0.0;      // eval_psi CULL (NMPC_CULL_RADIUS)
    Pools pools;                   // made by the first launch that needs them
    bool loop_order_prev = true;   // nmpc_loop_step: launch order from the previous step's pass counts (experiments: NMPC_LOOP_ORDER_PREV=0 switches it off)
    DevBuf<int> d_order;           // launch order (hard-looking instances first)
    bool use_order = true;
    DevBuf<unsigned char> d_cls;
    int order_n = 0;               // the last solve launch: instances it ordered (its B), 0 = it fetched in index order
    bool order_from_prev = false;  // ... and whether their levels came from the previous statuses
    Staging stg;
    SmallArena small;
    // wall-clock limits (nmpc_set_time_limits): as given, in ms, and in ticks of the 100 MHz constant clock (0 = off); any limit set -> the Timed<> kernels
    double tl_dur_ms = 0.0, tl_budget_ms = 0.0;
    long long tl_dur = 0, tl_budget = 0;
    DevBuf<long long> d_t0;        // the launch's start, written by nmpc_stamp_kernel when a budget is set (allocated with the first budget)
    std::string err;
};

// one clock reading on the device ahead of a launch with a batch budget: the start every instance's batch deadline counts from
__global__ void nmpc_stamp_kernel(long long *t0)
{
    if (threadIdx.x == 0) *t0 = (long long)__builtin_amdgcn_s_memrealtime();
}

extern "C" {

void nmpc_default_opts(nmpc_opts *o)
{
    o->tolerance = 1e-4;
    o->initial_tolerance = 1e-4;
    o->delta_tolerance = 1e-4;
    o->initial_penalty = 1.0;
    o->penalty_update = 5.0;
    o->tolerance_update = 0.1;
    o->sufficient_decrease = 0.1;
    o->lbfgs_memory = 10;
    o->max_inner = 500;
    o->max_outer = 10;
    o->max_total_inner = 0;
    o->akkt_gradient = 1;      // step_top: OpEn caches the previous gradient at the top of step()
    o->ls_failure = 0;
    o->inner_status = 0;
    o->reserved = 0;
}

int nmpc_n_u(const nmpc_problem *pb) { return 2 * pb->N; }
int nmpc_n1(const nmpc_problem *pb) { return 2 * pb->N; }
int nmpc_n2(const nmpc_problem *pb) { return pb->nobs + pb->ndyn; }
int nmpc_n_p(const nmpc_problem *pb) { return nmpc::NZ + pb->N + 3 * pb->nobs + 5 * pb->ndyn * pb->N + 3 * pb->N; }
int nmpc_abi_version(void) { return NMPC_ABI_VERSION; }
int nmpc_experiments_build(void)
{
#ifdef NMPC_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}

static int fail(nmpc_handle *h, int code, const char *what, hipError_t e = hipSuccess)
{
    if (h) {
        h->err = what;
        if (e != hipSuccess) { h->err += ": "; h->err += hipGetErrorString(e); }
    }
    return code;
}

#define HIP_TRY(h, call)                                                       \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) return fail((h), NMPC_ERR_HIP, #call, e_);       \
    } while (0)

static constexpr size_t LDS_PER_CU = 160 * 1024;      // bytes of LDS a gfx950 CU has: what one workgroup can ask for
static LdsMap make_map(const nmpc_problem &pb, int P) { return nmpc::lds_layout(pb.N, pb.nobs, pb.ndyn, P); }

// The knobs of the experiments build (csrc/variants/libnmpc_experiments.so), read once into a new handle: tests use them to check that
// every setting gives the same bits, scripts to measure.  The shipped library reads no environment.
static void read_knobs([[maybe_unused]] nmpc_handle *h)
{
#ifdef NMPC_EXPERIMENTS
    auto ival = [](const char *name, int &v) { if (const char *e = getenv(name)) v = atoi(e); };
    auto flag = [](const char *name, bool &v) { if (const char *e = getenv(name)) v = atoi(e) != 0; };
    auto pos = [](const char *name, double &v) { if (const char *e = getenv(name)) { const double x = atof(e); if (x > 0.0) v = x; } };
    if (const char *e = getenv("NMPC_SHAPE")) h->shape_any = !strcmp(e, "any");
    ival("NMPC_PARK_MIN", h->park_min);          // 0 switches the slot migration off
    ival("NMPC_PARK_DEPTH", h->park_depth);
    flag("NMPC_LOOP_ORDER_PREV", h->loop_order_prev);
    ival("NMPC_SCHED", h->sched_mode);
    pos("NMPC_SCHED_THETA", h->sched_theta);
    pos("NMPC_SCHED_COLD", h->sched_cold);
    pos("NMPC_CULL_RADIUS", h->cull_radius);
    flag("NMPC_TEAM_HELP", h->team_help);
    flag("NMPC_ORDER", h->use_order);            // 0 = instances in index order
    int owners = 0; ival("NMPC_TEAM_OWNERS", owners);
    if (owners >= 1 && owners <= nmpc::TEAM_WAVES) h->team_owners_forced = owners;
    ival("NMPC_WAVES_PER_CU", h->waves_per_cu);  // (nmpc_new keeps it only if it is a whole number of teams that fit)
    ival("NMPC_DEBUG_PRIO", h->dbg);
#endif
}

int nmpc_new(const nmpc_problem *pb, const nmpc_opts *opts, int device_id, int max_batch, nmpc_handle **out)
{
    if (!pb || !out || max_batch < 1) return NMPC_ERR_BAD_ARG;
    if (pb->N < 2 || pb->N > NMPC_MAX_HORIZON || pb->nobs < 0 || pb->nobs > 64 || pb->ndyn < 0 || pb->ndyn > nmpc::NDYN_MAX)
        return NMPC_ERR_BAD_PROBLEM;
    // ts and the boxes U and C (ranges stated in include/nmpc_solver.h); written so that a NaN fails every test
    auto finite = [](double x) { return x >= -DBL_MAX && x <= DBL_MAX; };
    if (!(pb->ts > 0.0 && pb->ts <= DBL_MAX) || !finite(pb->vmin) || !finite(pb->vmax) || !(pb->vmin <= pb->vmax) ||
        !finite(pb->amin) || !finite(pb->amax) || !(pb->amin <= pb->amax) ||
        !(pb->wmax >= 0.0 && pb->wmax <= DBL_MAX) || !(pb->awmax >= 0.0 && pb->awmax <= DBL_MAX))
        return NMPC_ERR_BAD_PROBLEM;
    nmpc_opts op;
    if (opts) op = *opts; else nmpc_default_opts(&op);
    if (op.lbfgs_memory < 1 || op.lbfgs_memory > nmpc::MAXMEM || op.max_inner < 1 || op.max_outer < 1 ||
        op.max_total_inner < 0 || op.akkt_gradient < 0 || op.akkt_gradient > 2 || op.ls_failure < 0 || op.ls_failure > 1 ||
        op.inner_status < 0 || op.inner_status > 1)
        return NMPC_ERR_BAD_OPTS;
    // the ALM knobs (ranges stated in include/nmpc_solver.h); written so that a NaN fails every test
    auto finite_pos = [](double x) { return x > 0.0 && x <= DBL_MAX; };
    if (!finite_pos(op.tolerance) || !finite_pos(op.initial_tolerance) || !finite_pos(op.delta_tolerance) ||
        !(op.initial_tolerance >= op.tolerance) || !finite_pos(op.initial_penalty) ||
        !(op.penalty_update > 1.0 && op.penalty_update <= DBL_MAX) ||
        !(op.tolerance_update > 0.0 && op.tolerance_update < 1.0) ||
        !(op.sufficient_decrease > 0.0 && op.sufficient_decrease < 1.0))
        return NMPC_ERR_BAD_OPTS;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev)
        return NMPC_ERR_NO_DEVICE;
    nmpc_handle *h = new nmpc_handle();
    h->pb = *pb; h->op = op; h->device = device_id; h->max_batch = max_batch;
    h->P = pb->N <= 20 ? 20 : 40;      // one stage per lane (nmpc_solve_hyb.h) / two stages per lane (nmpc_solve_hyb2.h); longer horizons are not served
    h->map = make_map(*pb, h->P == 40 ? 64 : h->P);      // (P = 40: the kernels compute their own map, nmpc_solve_hyb2.h)
    // long instances time-share beyond this fraction of the resident waves: the favoured half of them for the one-stage kernel (two waves per SIMD),
    // 0.8 for the two-stage kernel (one wave per SIMD); measured flat between 0.4 and 0.7 / 0.5 and 1.0 (profiles/r04/sched_sweep*.txt)
    h->sched_theta = h->P == 20 ? 0.5 : 0.8;
    // culling radius: what the input bounds let the robot travel in a horizon, plus a margin (any value is exact: an evaluation
    // with a stage beyond it scans every circle); NMPC_CULL_RADIUS overrides it (tests use 0.5 m: the fall-back runs all the time)
    h->cull_radius = 1.1 * pb->N * pb->ts * fmax(fabs(pb->vmin), fabs(pb->vmax));
    read_knobs(h);
    // the family's row specialised for this shape if there is one (and NMPC_SHAPE=any does not ask otherwise), else its run-time-shape row
    for (const SolveKernel &k : nmpc::SOLVE_KERNELS)
        if (k.P == h->P && (k.N == 0 ? !h->kernel[k.timed] : !h->shape_any && k.N == pb->N && k.nobs == pb->nobs && k.ndyn == pb->ndyn))
            h->kernel[k.timed] = &k;
    // one LDS slice per instance: the eval kernels hold three per wave, the solve kernels one per wave of a team of four plus the control block
    const size_t slice = (size_t)(h->P == 40 ? nmpc::lds_layout2(pb->N, pb->nobs, pb->ndyn).total : h->map.total) * sizeof(double);
    h->eval_lds = 3 * slice;
    h->team_lds = nmpc::TEAM_WAVES * slice + nmpc::TEAM_CTL_INTS * sizeof(int);
    if (h->eval_lds > LDS_PER_CU || h->team_lds > LDS_PER_CU) { nmpc_free(h); return NMPC_ERR_BAD_PROBLEM; }
    hipDeviceProp_t prop;
    hipError_t e = hipSetDevice(device_id);
    (void)hipGetDeviceProperties(&prop, device_id);
    if (e == hipSuccess) e = h->d_queue.alloc(1);
    if (e == hipSuccess) e = h->d_order.alloc(max_batch);
    if (e == hipSuccess) e = h->d_cls.alloc(max_batch);
    // more than 64 KB of dynamic LDS per workgroup has to be asked for
    for (const SolveKernel &k : nmpc::SOLVE_KERNELS)
        if (k.P == h->P && e == hipSuccess) e = hipFuncSetAttribute((const void *)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->team_lds);
    if (h->P == 40 && e == hipSuccess) e = hipFuncSetAttribute((const void *)nmpc::nmpc_eval2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->eval_lds);
    if (e != hipSuccess) { nmpc_free(h); return NMPC_ERR_HIP; }
    // resident waves per CU are bounded by LDS and by the register budget.  One stage per lane: two waves per SIMD, so up to two teams of
    // four waves; two stages per lane: one wave per SIMD (512 registers), the four waves of a CU are one team.
    int per_cu = nmpc::TEAM_WAVES * (h->P == 20 && 2 * h->team_lds <= LDS_PER_CU ? 2 : 1);
    if (h->waves_per_cu >= 1 && h->waves_per_cu <= per_cu && h->waves_per_cu % nmpc::TEAM_WAVES == 0) per_cu = h->waves_per_cu;
    h->grid_cap = prop.multiProcessorCount * per_cu;
    *out = h;
    return NMPC_OK;
}

void nmpc_free(nmpc_handle *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;      // (every buffer and event is released by its member's destructor)
}

int nmpc_ping(const nmpc_handle *h) { return (h && h->alive) ? NMPC_OK : NMPC_ERR_DEAD_HANDLE; }
const char *nmpc_last_error(const nmpc_handle *h) { return h ? h->err.c_str() : "null handle"; }
double nmpc_last_batch_ms(const nmpc_handle *h) { return h ? h->last_ms : 0.0; }
static bool timed(const nmpc_handle *h) { return h->tl_dur > 0 || h->tl_budget > 0; }
const char *nmpc_kernel_name(const nmpc_handle *h) { return h ? h->kernel[timed(h)]->name : ""; }
double nmpc_cull_radius(const nmpc_handle *h) { return h ? h->cull_radius : 0.0; }

static constexpr size_t PIN_CHUNK = 4u << 20;      // bytes of each pinned bounce buffer of the host path (h2d_staged / d2h_staged)
static nmpc::LaunchGeometry geometry_of(const nmpc_handle *h, int B)
{
    return nmpc::launch_geometry(B, h->grid_cap, h->P, h->use_order, h->park_min, h->sched_mode, h->team_owners_forced);
}
int nmpc_launch_geometry(const nmpc_handle *h, int B, nmpc_launch_info *out)
{
    if (!h || !out || B < 0 || B > h->max_batch) return NMPC_ERR_BAD_ARG;
    const nmpc::LaunchGeometry g = geometry_of(h, B);
    *out = nmpc_launch_info{g.grid, g.owners, g.workgroups, g.ordered, g.pools, g.pool_cap, h->grid_cap, 0, (int64_t)PIN_CHUNK};
    return NMPC_OK;
}

// a limit in ms -> ticks of the 100 MHz clock: 0 stays 0 (off), anything above it is at least one tick, and at most 2^52 ticks (16 months)
static long long ms_to_ticks(double ms)
{
    if (ms <= 0.0) return 0;
    const double t = ceil(ms * 1e5);
    const double cap = 4503599627370496.0;
    return t < 1.0 ? 1 : (long long)(t < cap ? t : cap);
}

int nmpc_set_time_limits(nmpc_handle *h, double max_duration_ms, double batch_budget_ms)
{
    if (!h) return NMPC_ERR_BAD_ARG;
    if (!h->alive) return NMPC_ERR_DEAD_HANDLE;
    // written so that a NaN fails the test: the limits in force stay as they are
    auto ok = [](double x) { return x >= 0.0 && x <= DBL_MAX; };
    if (!ok(max_duration_ms) || !ok(batch_budget_ms)) return fail(h, NMPC_ERR_BAD_OPTS, "time limits: negative, NaN or infinite");
    const long long budget = ms_to_ticks(batch_budget_ms);
    if (budget > 0 && !h->d_t0) {
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, h->d_t0.alloc(1));
    }
    h->tl_dur_ms = max_duration_ms; h->tl_budget_ms = batch_budget_ms;
    h->tl_dur = ms_to_ticks(max_duration_ms); h->tl_budget = budget;
    return NMPC_OK;
}

// what the batch entry points check first (NMPC_OK with B == 0: nothing to do)
static int check_batch(nmpc_handle *h, int B, const double *p, const double *u)
{
    if (!h) return NMPC_ERR_BAD_ARG;
    if (!h->alive) return NMPC_ERR_DEAD_HANDLE;
    if (B < 0 || B > h->max_batch || (B > 0 && (!p || !u))) return fail(h, NMPC_ERR_BAD_ARG, "bad batch arguments");
    return NMPC_OK;
}

static void fill_args(const nmpc_handle *h, KArgs &a, int B)
{
    std::memset(&a, 0, sizeof(a));
    a.pb = h->pb; a.op = h->op; a.map = h->map; a.B = B;
    a.n_p = nmpc_n_p(&h->pb); a.n_u = nmpc_n_u(&h->pb); a.n1 = nmpc_n1(&h->pb); a.n2 = nmpc_n2(&h->pb);
    a.queue = h->d_queue;
    a.inv_ts = 1.0 / h->pb.ts;
    a.dbg = h->dbg;
    a.tl_dur = h->tl_dur; a.tl_budget = h->tl_budget;
    a.tl_t0 = h->tl_budget > 0 ? h->d_t0.p : nullptr;
}

// the solve of nmpc_solve_batch_device.  prev: the statuses these very instances' previous solves left (nmpc_loop_step: launch order
// by their pass counts), or NULL: the order comes from the inputs
static int solve_launch(nmpc_handle *h, int B, const double *d_p, double *d_u, const double *d_y0, const double *d_c0, double *d_y_out,
                        nmpc_status *d_status, const nmpc_status *prev, void *stream)
{
    if (const int rc = check_batch(h, B, d_p, d_u); rc || B == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(h, hipSetDevice(h->device));
    KArgs a;
    fill_args(h, a, B);
    a.p = d_p; a.u = d_u; a.y0 = d_y0; a.c0 = d_c0; a.y_out = d_y_out; a.st = d_status;
    // a batch budget counts from one clock reading on the device, taken before anything of this launch runs (nothing is enqueued without one)
    if (h->tl_budget > 0) hipLaunchKernelGGL(nmpc_stamp_kernel, dim3(1), dim3(64), 0, s, h->d_t0.p);
    HIP_TRY(h, hipMemsetAsync(h->d_queue, 0, sizeof(unsigned int), s));
    // one instance per wave, three query points per pass: N_hor <= 20 with one stage per lane (hybrid / tri layouts), 20 < N_hor <= 40 with two
    const nmpc::LaunchGeometry geo = geometry_of(h, B);          // (nmpc_launch.h: the rule; nmpc_launch_geometry reports it)
    h->order_n = 0; h->order_from_prev = false;
    if (geo.ordered) {     // more instances than resident waves: hand the hard-looking ones out first
        h->order_n = B; h->order_from_prev = prev != nullptr;
        if (prev) hipLaunchKernelGGL(nmpc::nmpc_classify_prev_kernel, dim3((B + 255) / 256), dim3(256), 0, s, B, prev, h->d_cls.p);
        else hipLaunchKernelGGL(nmpc::nmpc_classify_kernel, dim3((B + 255) / 256), dim3(256), 0, s, a, h->d_cls.p);
        hipLaunchKernelGGL(nmpc::nmpc_order_kernel, dim3(1), dim3(1024), 0, s, B, h->d_cls.p, h->d_order.p);
        a.order = h->d_order;
    }
    if (geo.pools) {       // ... and instances may leave their wave at outer-iteration boundaries
        const size_t cap = (size_t)geo.pool_cap;      // ring buffers of this launch: an instance waits in at most one slot at a time
        const size_t cap_max = (size_t)h->max_batch;
        Pools &pl = h->pools;
        if (!pl.made()) {      // (all three or none: a half-made set is released and made again)
            pl.release();
            HIP_TRY(h, pl.park.alloc(cap_max * nmpc::park_stride(h->pb.N)));
            HIP_TRY(h, pl.pool.alloc(nmpc::NPOOLS * cap_max));
            HIP_TRY(h, pl.ctr.alloc(4 * nmpc::NPOOLS + 2));
        }
        HIP_TRY(h, hipMemsetAsync(pl.pool, 0xFF, nmpc::NPOOLS * cap * sizeof(int), s));
        HIP_TRY(h, hipMemsetAsync(pl.ctr, 0, (4 * nmpc::NPOOLS + 2) * sizeof(unsigned int), s));
        a.park_min = h->P == 20 ? h->park_min : 0; a.park_depth = h->park_depth;      // (the slot migration is the one-stage kernel's: two waves per SIMD)
        a.park = pl.park; a.pool = pl.pool; a.pool_ctr = pl.ctr; a.pool_cap = (int)cap;
        a.sched_mode = h->sched_mode;
    }
    {
        // teams of four waves, geo.owners of them taking instances (nmpc_launch.h)
        a.team_owners = geo.owners;
        a.sched_long_cap = (int)(h->sched_theta * (double)(geo.workgroups * geo.owners));
        a.sched_cold_cap = (int)(h->sched_cold * (double)(geo.workgroups * geo.owners));
        a.team_help = h->team_help;
        a.cull_radius = h->cull_radius;
        // (with a limit set: the same kernel with the wall-clock test compiled in, nmpc_set_time_limits)
        hipLaunchKernelGGL(h->kernel[timed(h)]->fn, dim3(geo.workgroups), dim3(64 * nmpc::TEAM_WAVES), h->team_lds, s, a);
    }
    HIP_TRY(h, hipGetLastError());
    return NMPC_OK;
}

int nmpc_solve_batch_device(nmpc_handle *h, int B, const double *d_p, double *d_u, const double *d_y0,
                            const double *d_c0, double *d_y_out, nmpc_status *d_status, void *stream)
{
    return solve_launch(h, B, d_p, d_u, d_y0, d_c0, d_y_out, d_status, nullptr, stream);
}

int nmpc_eval_batch_device(nmpc_handle *h, int B, const double *d_p, const double *d_u, const double *d_c,
                           const double *d_y, double *d_psi, double *d_grad, double *d_F1, double *d_F2,
                           void *stream)
{
    if (const int rc = check_batch(h, B, d_p, d_u); rc || B == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(h, hipSetDevice(h->device));
    KArgs a;
    fill_args(h, a, B);
    a.p = d_p; a.u = const_cast<double *>(d_u);
    a.ev_c = d_c; a.ev_y = d_y; a.ev_psi = d_psi; a.ev_grad = d_grad; a.ev_F1 = d_F1; a.ev_F2 = d_F2;
    const dim3 grid((B + 2) / 3);          // three instances per wave (the tri layout; two stages per lane for P = 40)
    if (h->P == 40) hipLaunchKernelGGL(nmpc::nmpc_eval2_kernel, grid, dim3(64), h->eval_lds, s, a);
    else hipLaunchKernelGGL(nmpc::nmpc_eval_kernel<20>, grid, dim3(64), h->eval_lds, s, a);
    HIP_TRY(h, hipGetLastError());
    return NMPC_OK;
}

// ---- host path: staging buffers sized for max_batch, allocated on first use ----
static int ensure_staging(nmpc_handle *h)
{
    Staging &g = h->stg;
    if (g.ready) return NMPC_OK;
    if (g.p) return fail(h, NMPC_ERR_HIP, "staging buffers: an earlier allocation failed half way");
    const size_t B = (size_t)h->max_batch;
    const size_t np = nmpc_n_p(&h->pb), nu = nmpc_n_u(&h->pb), n1 = nmpc_n1(&h->pb), n2 = nmpc_n2(&h->pb) + 1;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, g.p.alloc(B * np));
    HIP_TRY(h, g.u.alloc(B * nu));
    HIP_TRY(h, g.y0.alloc(B * n1));
    HIP_TRY(h, g.c0.alloc(B));
    HIP_TRY(h, g.yout.alloc(B * n1));
    HIP_TRY(h, g.psi.alloc(B));
    HIP_TRY(h, g.grad.alloc(B * nu));
    HIP_TRY(h, g.F1.alloc(B * n1));
    HIP_TRY(h, g.F2.alloc(B * n2));
    HIP_TRY(h, g.st.alloc(B));
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(h, g.pin[k].alloc(PIN_CHUNK));
        HIP_TRY(h, g.ev[k].create(hipEventDisableTiming));
    }
    g.ready = true;
    return NMPC_OK;
}

// Host buffers of the caller are pageable: a plain hipMemcpy moves them at ~3 GB/s.  They go through two pinned 4 MB bounce
// buffers instead -- the CPU fills one while the DMA engine drains the other -- in stream order with the kernels (null stream).
static hipError_t h2d_staged(nmpc_handle *h, void *dst, const void *src, size_t bytes)
{
    hipError_t e = hipSuccess;
    int k = 0;
    for (size_t off = 0; off < bytes && e == hipSuccess; off += PIN_CHUNK, k ^= 1) {
        const size_t n = bytes - off < PIN_CHUNK ? bytes - off : PIN_CHUNK;
        e = hipEventSynchronize(h->stg.ev[k]);                       // (the copy that last used this buffer; a fresh event is complete)
        if (e != hipSuccess) break;
        std::memcpy(h->stg.pin[k], (const char *)src + off, n);
        e = hipMemcpyAsync((char *)dst + off, h->stg.pin[k], n, hipMemcpyHostToDevice, nullptr);
        if (e == hipSuccess) e = hipEventRecord(h->stg.ev[k], nullptr);
    }
    return e;
}
static hipError_t d2h_staged(nmpc_handle *h, void *dst, const void *src, size_t bytes)
{
    hipError_t e = hipSuccess;
    size_t pend_off[2] = {0, 0}, pend_n[2] = {0, 0};
    int k = 0;
    for (size_t off = 0; off < bytes && e == hipSuccess; off += PIN_CHUNK, k ^= 1) {
        const size_t n = bytes - off < PIN_CHUNK ? bytes - off : PIN_CHUNK;
        if (pend_n[k]) {                                             // drain what this buffer still holds
            e = hipEventSynchronize(h->stg.ev[k]);
            if (e != hipSuccess) break;
            std::memcpy((char *)dst + pend_off[k], h->stg.pin[k], pend_n[k]);
        }
        e = hipMemcpyAsync(h->stg.pin[k], (const char *)src + off, n, hipMemcpyDeviceToHost, nullptr);
        if (e == hipSuccess) e = hipEventRecord(h->stg.ev[k], nullptr);
        pend_off[k] = off; pend_n[k] = n;
    }
    for (int j = 0; j < 2 && e == hipSuccess; ++j, k ^= 1)           // the last one or two chunks, oldest first
        if (pend_n[k]) {
            e = hipEventSynchronize(h->stg.ev[k]);
            if (e == hipSuccess) std::memcpy((char *)dst + pend_off[k], h->stg.pin[k], pend_n[k]);
            pend_n[k] = 0;
        }
    return e;
}

static constexpr int SMALL_BATCH = 16;      // instances the small-batch arena holds
static int solve_small_host(nmpc_handle *h, int B, const double *p, double *u, const double *y0, const double *c0,
                            double *y_out, nmpc_status *status)
{
    const size_t np = nmpc_n_p(&h->pb), nu = nmpc_n_u(&h->pb), n1 = nmpc_n1(&h->pb);
    const size_t cap = SMALL_BATCH;
    const size_t o_p = 0, o_c = o_p + cap * np * 8, o_y = o_c + cap * 8, o_u = o_y + cap * n1 * 8, o_yo = o_u + cap * nu * 8,
                 o_st = o_yo + cap * n1 * 8, total = o_st + cap * sizeof(nmpc_status);
    HIP_TRY(h, hipSetDevice(h->device));
    SmallArena &g = h->small;
    if (!g.ready) {
        // all or none: what an earlier, failed attempt left behind is released first, so a transient failure costs one call, not the handle's small-batch path
        g.release();
        HIP_TRY(h, g.d.alloc(total));
        HIP_TRY(h, g.h.alloc(total));
        for (int k = 0; k < 2; ++k) HIP_TRY(h, g.ev[k].create());
        g.ready = true;
    }
    char *hs = g.h, *ds = g.d;
    // in: p .. u of the B instances (each array at its arena offset; only what is used travels, as one copy from the first to the last byte used)
    std::memcpy(hs + o_p, p, B * np * 8);
    if (c0) std::memcpy(hs + o_c, c0, B * 8);
    if (y0) std::memcpy(hs + o_y, y0, B * n1 * 8);
    std::memcpy(hs + o_u, u, B * nu * 8);
    HIP_TRY(h, hipMemcpyAsync(ds, hs, o_u + B * nu * 8, hipMemcpyHostToDevice, nullptr));
    HIP_TRY(h, hipEventRecord(g.ev[0], nullptr));
    const int rc = nmpc_solve_batch_device(h, B, (const double *)(ds + o_p), (double *)(ds + o_u), y0 ? (const double *)(ds + o_y) : nullptr,
                                           c0 ? (const double *)(ds + o_c) : nullptr, (double *)(ds + o_yo), (nmpc_status *)(ds + o_st), nullptr);
    if (rc) return rc;
    HIP_TRY(h, hipEventRecord(g.ev[1], nullptr));
    HIP_TRY(h, hipMemcpyAsync(hs + o_u, ds + o_u, total - o_u, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(h, hipStreamSynchronize(nullptr));
    float ms = 0.f;
    HIP_TRY(h, hipEventElapsedTime(&ms, g.ev[0], g.ev[1]));
    h->last_ms = (double)ms;
    std::memcpy(u, hs + o_u, B * nu * 8);
    if (y_out) std::memcpy(y_out, hs + o_yo, B * n1 * 8);
    if (status) std::memcpy(status, hs + o_st, B * sizeof(nmpc_status));
    return NMPC_OK;
}

int nmpc_solve_batch_host(nmpc_handle *h, int B, const double *p, double *u, const double *y0, const double *c0,
                          double *y_out, nmpc_status *status)
{
    if (const int rc = check_batch(h, B, p, u); rc || B == 0) return rc;
    if (B <= SMALL_BATCH) return solve_small_host(h, B, p, u, y0, c0, y_out, status);
    int rc = ensure_staging(h);
    if (rc) return rc;
    const Staging &g = h->stg;
    const size_t np = nmpc_n_p(&h->pb), nu = nmpc_n_u(&h->pb), n1 = nmpc_n1(&h->pb);
    HIP_TRY(h, h2d_staged(h, g.p, p, B * np * 8));
    HIP_TRY(h, h2d_staged(h, g.u, u, B * nu * 8));
    if (y0) HIP_TRY(h, h2d_staged(h, g.y0, y0, B * n1 * 8));
    if (c0) HIP_TRY(h, h2d_staged(h, g.c0, c0, B * 8));
    Event e0, e1;
    float ms = 0.f;
    hipError_t he = e0.create();
    if (he == hipSuccess) he = e1.create();
    if (he == hipSuccess) he = hipEventRecord(e0, nullptr);
    if (he == hipSuccess) {
        rc = nmpc_solve_batch_device(h, B, g.p, g.u, y0 ? g.y0.p : nullptr, c0 ? g.c0.p : nullptr,
                                     g.yout, g.st, nullptr);
        if (rc == NMPC_OK) {
            he = hipEventRecord(e1, nullptr);
            if (he == hipSuccess) he = hipDeviceSynchronize();
            if (he == hipSuccess) he = hipEventElapsedTime(&ms, e0, e1);
        }
    }
    if (rc) return rc;
    if (he != hipSuccess) return fail(h, NMPC_ERR_HIP, "solve_batch_host", he);
    h->last_ms = (double)ms;
    HIP_TRY(h, d2h_staged(h, u, g.u, B * nu * 8));
    if (y_out) HIP_TRY(h, d2h_staged(h, y_out, g.yout, B * n1 * 8));
    if (status) HIP_TRY(h, d2h_staged(h, status, g.st, B * sizeof(nmpc_status)));
    return NMPC_OK;
}

int nmpc_eval_batch_host(nmpc_handle *h, int B, const double *p, const double *u, const double *c, const double *y,
                         double *psi, double *grad, double *F1, double *F2)
{
    if (const int rc = check_batch(h, B, p, u); rc || B == 0) return rc;
    int rc = ensure_staging(h);
    if (rc) return rc;
    const Staging &g = h->stg;
    const size_t np = nmpc_n_p(&h->pb), nu = nmpc_n_u(&h->pb), n1 = nmpc_n1(&h->pb), n2 = nmpc_n2(&h->pb);
    HIP_TRY(h, h2d_staged(h, g.p, p, B * np * 8));
    HIP_TRY(h, h2d_staged(h, g.u, u, B * nu * 8));
    if (y) HIP_TRY(h, h2d_staged(h, g.y0, y, B * n1 * 8));
    if (c) HIP_TRY(h, h2d_staged(h, g.c0, c, B * 8));
    rc = nmpc_eval_batch_device(h, B, g.p, g.u, c ? g.c0.p : nullptr, y ? g.y0.p : nullptr, g.psi,
                                g.grad, g.F1, g.F2, nullptr);
    if (rc) return rc;
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, g.psi.read(psi, B));
    HIP_TRY(h, g.grad.read(grad, B * nu));
    HIP_TRY(h, g.F1.read(F1, B * n1));
    if (n2) HIP_TRY(h, g.F2.read(F2, B * n2));
    return NMPC_OK;
}

// ---- receding-horizon loop on device (kernels: nmpc_loop.h) and a route per robot, planned on device (kernels: nmpc_plan.h) ----
#include "nmpc_loop_host.h"
#include "nmpc_plan_host.h"

// ---- arithmetic primitives, for bit-level checks against the oracle ----
__global__ void nmpc_test_sincos_kernel(int n, const double *x, double *s, double *c)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) nmpc::sincos_cw(x[i], s[i], c[i]);
}
__global__ void nmpc_test_divsqrt_kernel(int n, const double *a, const double *b, double *q, double *r)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { q[i] = a[i] / b[i]; r[i] = sqrt(a[i]); }
}

static int run_unary_test(nmpc_handle *h, int n, const double *x0, const double *x1, double *o0, double *o1, int which)
{
    if (!h || n < 0 || !x0 || !o0 || !o1) return NMPC_ERR_BAD_ARG;
    if (n == 0) return NMPC_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    DevBuf<double> d[4];
    hipError_t e = hipSuccess;
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = d[i].alloc(n);
    if (e == hipSuccess) e = hipMemcpy(d[0], x0, (size_t)n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && x1) e = hipMemcpy(d[1], x1, (size_t)n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const int blocks = (n + 255) / 256;
        if (which == 0) hipLaunchKernelGGL(nmpc_test_sincos_kernel, dim3(blocks), dim3(256), 0, nullptr, n, d[0].p, d[2].p, d[3].p);
        else hipLaunchKernelGGL(nmpc_test_divsqrt_kernel, dim3(blocks), dim3(256), 0, nullptr, n, d[0].p, d[1].p, d[2].p, d[3].p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(o0, d[2], (size_t)n * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(o1, d[3], (size_t)n * 8, hipMemcpyDeviceToHost);
    return e == hipSuccess ? NMPC_OK : fail(h, NMPC_ERR_HIP, "arithmetic primitive test", e);
}

int nmpc_test_sincos_host(nmpc_handle *h, int n, const double *x, double *out_s, double *out_c)
{
    return run_unary_test(h, n, x, nullptr, out_s, out_c, 0);
}
int nmpc_test_divsqrt_host(nmpc_handle *h, int n, const double *a, const double *b, double *out_div, double *out_sqrt)
{
    if (!b) return NMPC_ERR_BAD_ARG;
    return run_unary_test(h, n, a, b, out_div, out_sqrt, 1);
}

// ---- the launch order, readable in the experiments build only (tests/test_gpu_launch_order.py); include/nmpc_solver.h declares neither and
// the product exports neither ----
#ifdef NMPC_EXPERIMENTS
// what the handle's last solve launch used, after the device has finished it: *n = its B, or 0 if it fetched in index order (B within the
// resident waves, or NMPC_ORDER=0); *from_prev = the levels came from statuses; cls[0..n), order[0..n) (either may be NULL)
int nmpc_debug_launch_order(nmpc_handle *h, int32_t *n, int32_t *from_prev, uint8_t *cls, int32_t *order)
{
    if (!h || !n || !from_prev) return NMPC_ERR_BAD_ARG;
    if (!h->alive) return NMPC_ERR_DEAD_HANDLE;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    *n = h->order_n; *from_prev = h->order_from_prev ? 1 : 0;
    HIP_TRY(h, h->d_cls.read(cls, (size_t)h->order_n));
    HIP_TRY(h, h->d_order.read(order, (size_t)h->order_n));
    return NMPC_OK;
}

// the order of B instances whose previous solves took passes[b] evaluation passes: the two kernels solve_launch enqueues for a launch with
// statuses, on the handle's own buffers (so the record of the last launch is cleared), without a solve behind them
int nmpc_debug_order_of(nmpc_handle *h, int B, const uint32_t *passes, uint8_t *cls, int32_t *order)
{
    if (!h || !passes) return NMPC_ERR_BAD_ARG;
    if (!h->alive) return NMPC_ERR_DEAD_HANDLE;
    if (B < 1 || B > h->max_batch) return fail(h, NMPC_ERR_BAD_ARG, "bad batch arguments");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    std::vector<nmpc_status> st((size_t)B);
    std::memset(st.data(), 0, st.size() * sizeof(nmpc_status));
    for (int b = 0; b < B; ++b) st[b].reserved = passes[b];
    DevBuf<nmpc_status> prev;
    HIP_TRY(h, prev.upload(st.data(), st.size()));
    h->order_n = 0; h->order_from_prev = false;
    hipLaunchKernelGGL(nmpc::nmpc_classify_prev_kernel, dim3((B + 255) / 256), dim3(256), 0, nullptr, B, prev.p, h->d_cls.p);
    hipLaunchKernelGGL(nmpc::nmpc_order_kernel, dim3(1), dim3(1024), 0, nullptr, B, h->d_cls.p, h->d_order.p);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, h->d_cls.read(cls, (size_t)B));
    HIP_TRY(h, h->d_order.read(order, (size_t)B));
    return NMPC_OK;
}
#endif

}  // extern "C"

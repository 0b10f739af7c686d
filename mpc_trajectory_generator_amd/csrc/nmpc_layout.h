// nmpc_layout.h -- constants, the launch arguments (KArgs), problem shapes, the LDS slice map and the set-up of an instance in its slice.
#pragma once

#ifndef NMPC_WIN
#define NMPC_WIN 1      // half width of the cross-track window of the one-stage-per-lane kernels (eval_psi); 0 = always the full scan
#endif

namespace nmpc {

constexpr int NZ = 20;         // reference configs/default.yaml:35
constexpr int MAXMEM = 10;     // L-BFGS memory the kernel is built for
constexpr int NDYN_MAX = 3;    // Ndynobs the kernel is built for
constexpr int GRAM_LD = 11;    // row stride of the kept inner products gsy / gyy (doubles): with 10 the ten lanes of a column read hit 8 bank pairs, with 11 ten
constexpr int GRAM_NST = 20;   // stages the Gram-form L-BFGS of the hybrid kernel runs over (N_hor <= 20, zero padded)
constexpr int OBS_STRIDE = 4;  // doubles per static circle in LDS: xs ys r^2 r
constexpr int SEG_STRIDE = 5;  // doubles per reference segment in LDS (odd: the per-lane window gathers of eval_psi spread over all banks)
// team mode of the hybrid kernel (nmpc_solve_hyb.h): four waves per workgroup; a wave without work of its own evaluates
// line-search trials for its siblings.  Request = u, r, d by stage (3 x 24 pairs); one result area = three trials'
// gradients by stage (3 x 24 pairs) + their psi values
constexpr int TEAM_WAVES = 4;
constexpr int TEAM_REQ_DOUBLES = 3 * 24 * 2;
constexpr int TEAM_AREA_DOUBLES = 3 * 24 * 2 + 8;     // + psi[3], envelope[3]
constexpr int TEAM_CTL_INTS = 64;
// instances waiting for a wave (nmpc_solve_hyb.h): long = an outer criterion is still open after the outer iteration just finished, cold = all hold: the next outer iteration is the last (and short)
constexpr int NPOOLS = 2;
enum { POOL_LONG = 0, POOL_COLD = 1 };

// PANOC constants
constexpr double GAMMA_L_COEFF = 0.95;
constexpr double DELTA_LIPSCHITZ = 1e-12;
constexpr double EPSILON_LIPSCHITZ = 1e-6;
constexpr double LIPSCHITZ_UPDATE_EPSILON = 1e-6;
constexpr int MAX_LIPSCHITZ_UPDATE_ITERATIONS = 10;
constexpr double MAX_LIPSCHITZ_CONSTANT = 1e9;
constexpr double MIN_LIPSCHITZ_CONSTANT = 1e-10;
constexpr int MAX_LINESEARCH_ITERATIONS = 10;
constexpr double LBFGS_SY_EPSILON = 1e-10;
constexpr double LBFGS_CBFGS_EPSILON = 1e-8;

// LDS slice of one group (offsets in doubles)
struct LdsMap {
    int sc;      // 18 instance scalars: x0 y0 th0 vinit winit xf yf thf | q qv qth rv rw qN qthN qcte pa pw | vinit winit again, as an aligned pair
    int cw;      // CW_NCOEF sin/cos polynomial coefficients (nmpc_device.h)
    int par;     // up to 24 parked solver scalars (hybrid kernel)
    int seg;     // SEG_STRIDE = 5 per reference segment (40 B): s1x s1y dx dy 1/(|d|^2 + 1e-16)
    int obs;     // OBS_STRIDE per static circle: xs ys r^2 r
    int f2;      // n2 penalty values
    int dyn;     // NDYN_MAX x 6 x dyn_stride per-stage ellipse data
    int dyn_stride;  // columns per (ellipse, field): 24 / 32 for the three- / two-point layouts, N rounded up to even for one point
    int req;     // hybrid kernel, team mode: the line-search request of this wave's instance -- u, r, d as 3 x 24 (v, w) pairs by stage
    int vec;     // 7 x P parked (v, w) pairs: L-BFGS old u / old r, previous gradient, y+, y, reference speed, grad at u_k
    int rho;     // m
    int S, Y;    // m slots x N lanes x (v, w)
    int nv;      // hybrid kernel, Gram-form L-BFGS: the four vectors of an iteration -- s | y | r | g -- as 4 x GRAM_NST (v, w) pairs by stage
    int gsy, gyy; // ... and the inner products it keeps, [slot][slot]: <s_a, y_b> (a older than b; zero otherwise), <y_a, y_b>
    int total;
};

struct KArgs {
    nmpc_problem pb;
    nmpc_opts op;
    LdsMap map;
    int B;
    int n_p, n_u, n1, n2;
    double inv_ts;
    const double *p;
    double *u;
    const double *y0;
    const double *c0;
    double *y_out;
    nmpc_status *st;
    unsigned int *queue;
    const int *order;          // queue position -> instance (longest-expected-first), or NULL = index order
    // migration of long-running instances to the SIMD's favoured wave slot (nmpc_solve_hyb.h), 0 = off
    int park_min;              // passes after which an instance on an unfavoured wave is parked at an outer-iteration boundary
    int park_depth;            // ... unless this many parked instances are already waiting for a favoured wave
    double *park;              // [B][park_stride]: parked solver state
    int *pool;                 // [B]: parked instance ids in arrival order (-1: not yet published)
    unsigned int *pool_ctr;    // per pool: head, tail, count, pad (nmpc_solve_hyb.h: POOL_CTRS); after the pools: instances alive that are known to be long
    int pool_cap;              // slots per pool ring (>= B)
    int sched_mode;            // 0: an instance stays on its wave (but for the slot migration); 1: step-aside scheduling at outer-iteration boundaries (nmpc_solve_hyb.h)
    int sched_long_cap;        // long instances alive beyond this many time-share the waves
    int sched_cold_cap;        // cold instances step aside once this many long instances are alive (a batch without long instances has nobody to make room for)
    int dbg;                   // experiments (NMPC_DEBUG_PRIO): static wave priorities + per-instance cycle counts
    int team_owners;           // hybrid kernel: waves per workgroup that take instances from the queue (1..4); the others only help
    int team_help;             // 0: nobody asks for help (experiments, NMPC_TEAM_HELP=0: the single-wave baseline)
    double cull_radius;        // eval_psi's CULL path: circles whose edge is farther than this from the start position are left out of the scan
    // (a launch is an evaluation or a solve: their own arguments share the room, so that the argument block keeps its size and layout)
    union {
        struct {           // eval kernel only
            const double *ev_c;
            const double *ev_y;
            double *ev_psi, *ev_grad, *ev_F1, *ev_F2;
        };
        struct {           // wall-clock limits (nmpc_set_time_limits; read by the Timed<> solve kernels only), in ticks of the 100 MHz constant clock, 0 = off
            long long tl_dur;          // per instance, from its first start
            long long tl_budget;       // per launch, from *tl_t0
            const long long *tl_t0;    // the launch's start, stamped on the device ahead of the solve (nmpc_stamp_kernel); NULL without a budget
        };
    };
};

enum { SC_X0 = 0, SC_Y0, SC_TH0, SC_VINIT, SC_WINIT, SC_XF, SC_YF, SC_THF,
       SC_Q, SC_QV, SC_QTH, SC_RV, SC_RW, SC_QN, SC_QTHN, SC_QCTE, SC_PA, SC_PW };

// LDS pointers carry their address space: no generic-pointer casts, always ds_* instructions
typedef __attribute__((address_space(3))) double lds_double;
typedef double dbl2 __attribute__((ext_vector_type(2)));     // (v, w) pair, 16-byte aligned
typedef __attribute__((address_space(3))) dbl2 lds_double2;

#ifdef NMPC_NO_SCHED_BARRIER
#define NMPC_SCHED_BARRIER() do { } while (0)
#else
#define NMPC_SCHED_BARRIER() __builtin_amdgcn_sched_barrier(0)
#endif
#define NMPC_WAVE_SYNC()                                           \
    do {                                                           \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");     \
        __builtin_amdgcn_wave_barrier();                           \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");     \
    } while (0)

// per-stage data of the dynamic ellipses: six values per (ellipse, stage), kept in the LDS slice as
// [ellipse][field][stage] so the stage's lane reads its column conflict-free
enum { DY_EX = 0, DY_EY, DY_CA, DY_SA, DY_IRX2, DY_IRY2, DY_FIELDS };
struct DynStage {
    const lds_double *col;     // this lane's column
    int stride;                // lanes per group (P)
    __device__ __forceinline__ double get(int k, int f) const { return col[(k * DY_FIELDS + f) * stride]; }
};

// Problem shape known at compile time (0 / -1: taken from the arguments at run time).  The reference
// generates one solver per configuration (mpc_generator.py:173-193); ShapeDefault is the shape of
// configs/default.yaml (N_hor 20, Nobs 10, Ndynobs 3), for which loops unroll and LDS offsets fold.
struct ShapeAny { static constexpr int N = 0, NOBS = -1, NDYN = -1; };
struct ShapeDefault { static constexpr int N = 20, NOBS = 10, NDYN = 3; };
struct ShapeNobs50 { static constexpr int N = 20, NOBS = 50, NDYN = 3; };     // BASELINE config 3
struct ShapeN40 { static constexpr int N = 40, NOBS = 10, NDYN = 3; };        // BASELINE config 2
// The same shape with the wall-clock limits of nmpc_set_time_limits compiled in: the solve kernels instantiated for Timed<S> test the
// device's 100 MHz clock where they test opts.max_total_inner; those for S itself hold no clock test and are the untimed kernels.
template <class S> struct Timed { static constexpr int N = S::N, NOBS = S::NOBS, NDYN = S::NDYN; };
template <class SH> struct ShapeTimed { static constexpr bool value = false; };
template <class S> struct ShapeTimed<Timed<S>> { static constexpr bool value = true; };
template <class SH> __device__ __forceinline__ int shape_N(const KArgs &a) { if constexpr (SH::N > 0) return SH::N; else return a.pb.N; }
template <class SH> __device__ __forceinline__ int shape_nobs(const KArgs &a) { if constexpr (SH::NOBS >= 0) return SH::NOBS; else return a.pb.nobs; }
template <class SH> __device__ __forceinline__ int shape_ndyn(const KArgs &a) { if constexpr (SH::NDYN >= 0) return SH::NDYN; else return a.pb.ndyn; }

// The LDS slice layout (offsets in doubles) as a function of the problem shape and the lane layout P (20: three query points
// per wave, 32: two, 64: one).  constexpr: the shape-specialised kernels fold every offset into the ds_* instructions'
// immediate fields instead of carrying a dozen kernel arguments in (spilled) SGPRs; the host computes the same map for the
// run-time-shape kernels and for sizing the launch.  The L-BFGS ring is sized for MAXMEM slots whatever opts.lbfgs_memory is.
__host__ __device__ constexpr LdsMap lds_layout(int N, int nobs, int ndyn, int P)
{
    LdsMap mp{};
    int o = 0;
    mp.sc = o;  o += 20;
    mp.cw = o;  o += CW_NCOEF;
    mp.par = o; o += 24;
    mp.seg = o; o += SEG_STRIDE * (N + 5);
    mp.obs = o; o += OBS_STRIDE * (nobs + 4);
    const int points = P == 64 ? 1 : 3;               // F2 arrays: one per query point of a pass (eval kernel: per group slice)
    // (three-point layout: only the cost-layer kernel writes F2, and it has no parked vectors -- the array shares their place)
    mp.f2 = o;  o += P == 20 ? 0 : points * (nobs + ndyn + 1);
    mp.rho = o; o += MAXMEM;
    const int cols = P == 20 ? 24 : P;                // >= lay_cols (hybrid kernel: state lanes 24..31 share column 23 -- all zeros)
    // one point per wave keeps its solver vectors in registers and needs ellipse columns for the real stages only: without
    // the 64-column tables a 40-stage slice is 21.6 KB instead of 32.9 KB -- 7 resident waves per CU instead of 4
    mp.dyn_stride = P == 64 ? ((N + 1) & ~1) : (P == 20 ? 24 : P);
    mp.dyn = o; o += NDYN_MAX * 6 * mp.dyn_stride;
    o = (o + 1) & ~1;
    mp.req = o; o += P == 20 ? TEAM_REQ_DOUBLES : 0;
    mp.vec = o; o += P == 64 ? 0 : 7 * 2 * cols;
    if (P == 20) { mp.f2 = mp.vec; if (7 * 2 * cols < points * (nobs + ndyn + 1)) o = mp.vec + points * (nobs + ndyn + 1); }
    o = (o + 1) & ~1;                                 // 16-byte alignment for the double2 arrays
    // hybrid kernel: GRAM_NST + 1 columns per slot whatever N is -- the Gram batch reads a slot as GRAM_NST pairs, the last column is
    // all zeros (lanes beyond the horizon read it); gsy | gyy | S | Y are contiguous (zeroed together when the buffer is reset)
    mp.gsy = o; o += P == 20 ? MAXMEM * GRAM_LD : 0;
    mp.gyy = o; o += P == 20 ? MAXMEM * GRAM_LD : 0;
    const int ring = P == 20 ? GRAM_NST + 1 : N;
    mp.S = o;   o += 2 * ring * MAXMEM;
    mp.Y = o;   o += 2 * ring * MAXMEM;
    mp.nv = o;  o += P == 20 ? 4 * 2 * GRAM_NST : 0;
    mp.total = (o + 1) & ~1;
    // team mode: a helper wave's slice holds one result area per (owner, task) from offset 0 -- twelve of them; short horizons make slices
    // smaller than that (N_hor <= 14), and an area past the slice would land in the next wave's tables
    if (P == 20 && mp.total < 3 * TEAM_WAVES * TEAM_AREA_DOUBLES) mp.total = 3 * TEAM_WAVES * TEAM_AREA_DOUBLES;
    return mp;
}
// the map a kernel instantiation works with: compile-time for a fixed shape, the launch argument otherwise
template <class SH, int P> __device__ __forceinline__ LdsMap the_map(const KArgs &a)
{
    if constexpr (SH::N > 0 && SH::NOBS >= 0 && SH::NDYN >= 0) return lds_layout(SH::N, SH::NOBS, SH::NDYN, P);
    else return a.map;
}

// ---------------------------------------------------------------------------------------------
// instance set-up: p -> LDS slice + per-lane registers     (reference mpc_generator.py:73-79,93-104,127-136)
// ---------------------------------------------------------------------------------------------
template <int P, class SH = ShapeAny>
__device__ __forceinline__ void prepare_instance(const KArgs &a, lds_double *L, const double *p, int t,
                                                 double &vref, DynStage &dyn)
{
    const int N = shape_N<SH>(a), nobs = shape_nobs<SH>(a), ndyn = shape_ndyn<SH>(a);
    const LdsMap mp = the_map<SH, P>(a);
    if (t < 8) L[mp.sc + t] = p[t];                      // state, last input, target (p[8:10] unused)
    if (t >= 8 && t < 18) L[mp.sc + t] = p[t + 2];       // ten weights p[10:20]
    if (t == 18 || t == 19) L[mp.sc + t] = p[t - 15];    // the last input once more, as a (v, w) pair: "the stage before stage 0" of the hybrid kernel's transport
    if (t < CW_NCOEF) L[mp.cw + t] = CW_COEF_DEV[t];
    NMPC_WAVE_SYNC();
    vref = t < N ? p[NZ + t] : 0.0;
    const double *ps = p + NZ + N;
    for (int k = t; k < ((nobs + 4) & ~3); k += P) {       // padded to a multiple of 4 with inert zero circles (slot `nobs` always is one)
        const bool real = k < nobs;
        const double r = real ? ps[3 * k + 2] : 0.0;
        L[mp.obs + OBS_STRIDE * k] = real ? ps[3 * k] : 0.0;
        L[mp.obs + OBS_STRIDE * k + 1] = real ? ps[3 * k + 1] : 0.0;
        L[mp.obs + OBS_STRIDE * k + 2] = r * r;
        L[mp.obs + OBS_STRIDE * k + 3] = r > 0.0 ? r : -1e30;      // (obstacle certificate: an empty slot is infinitely far away)
    }
    const double *pd = ps + 3 * nobs;
    {
        lds_double *col = L + mp.dyn + t;
        dyn.col = col;
        // one point per wave (P = 64): only the N real stages have a column (the slice then fits 7 waves per CU, not 4)
        const int ds = P == 64 ? mp.dyn_stride : lay_cols<P>();
        dyn.stride = ds;
#pragma unroll
        for (int k = 0; k < NDYN_MAX; ++k) {
            double ex = 0.0, ey = 0.0, ca = 0.0, sa = 0.0, irx2 = 1.0, iry2 = 1.0;
            if (k < ndyn && t < N) {
                const double *e = pd + (k * N + t) * 5;
                ex = e[0];
                ey = e[1];
                irx2 = 1.0 / (e[2] * e[2]);
                iry2 = 1.0 / (e[3] * e[3]);
                sincos_cw_t(e[4], (const lds_double *)(L + mp.cw), sa, ca);
            }
            if (P != 64 || t < ds) {
                col[(k * DY_FIELDS + DY_EX) * ds] = ex;
                col[(k * DY_FIELDS + DY_EY) * ds] = ey;
                col[(k * DY_FIELDS + DY_CA) * ds] = ca;
                col[(k * DY_FIELDS + DY_SA) * ds] = sa;
                col[(k * DY_FIELDS + DY_IRX2) * ds] = irx2;
                col[(k * DY_FIELDS + DY_IRY2) * ds] = iry2;
            }
        }
    }
    const double *pr = pd + 5 * ndyn * N;
    const int nseg4 = (N - 1 + 3) & ~3;                    // the CTE loop runs 4 segments per trip; the padding
    if (t < nseg4) {                                       // repeats the last segment (cannot change a strict min)
        const int i = t < N - 1 ? t : N - 2;
        const double ax = pr[3 * i], ay = pr[3 * i + 1];
        const double bx = pr[3 * i + 3], by = pr[3 * i + 4];
        const double dx = bx - ax, dy = by - ay;
        lds_double *sg = L + mp.seg + SEG_STRIDE * t;
        sg[0] = ax;
        sg[1] = ay;
        sg[2] = dx;
        sg[3] = dy;
        sg[4] = 1.0 / (fma(dx, dx, dy * dy) + 1e-16);
    }
    NMPC_WAVE_SYNC();
}

// doubles per parked instance: u, y, previous gradient (2N each) + 16 scalars
__host__ __device__ inline int park_stride(int N) { return 6 * N + 16; }
}  // namespace nmpc

// nmpc_eval.h -- psi, grad psi, F1, F2 at a point held one stage per lane (eval_psi, its window and obstacle certificate), the cost-layer kernel.
#pragma once

namespace nmpc {

// Windowed cross-track search (eval_psi / eval_psi2, WIN > 0).  What a lane remembers from its last FULL scan of the reference segments:
// the centre of its window, where the stage was then, and the squared distance from there to the nearest segment OUTSIDE the window
// (0 = nothing known: the next evaluation scans everything).
struct WinState {
    int ctr;
    double xr, yr, mo2;
};
// Obstacle certificate (eval_psi, oc != nullptr).  The activity scan of an evaluation only decides WHICH circles / ellipses have a stage of
// the wave inside them (the touched ones are then summed exactly); from one evaluation to the next that set rarely changes.  So a lane
// remembers where its stage was at the wave's last scan and how far that was -- at least -- from every obstacle the scan found
// untouched (distance to the circle's edge; for an ellipse to the disc of its larger half axis around its centre; for the culled scan
// also to the culling radius), and the wave remembers the scan's verdict.  While every stage has moved by less than its clearance no
// untouched obstacle can have been entered: the old verdict is a superset of the true one, and a superfluous member contributes exactly
// zero (its sum is +0.0, no lane is inside it) -- the scan is skipped and the result is bit for bit the scanning evaluation's.  The
// clearances come from v_sqrt_f64 / v_rsq_f64 (approximate) with 1 % + 1e-6 taken off: they only decide whether the scan runs.
struct ObsCert {
    double xo, yo, m2;             // this lane: the stage's position at the wave's last scan, squared clearance there (0: scan next time).  (A reference
                                   // point shared with the cross-track window was measured: four registers less, but either certificate's failure then
                                   // runs both scans -- 10 % of the evaluations instead of 1 %, headline + 6 %.)
    // the wave: circles and ellipses the last scan found touched.  Kept in VECTOR registers (every lane the same value; read back with
    // v_readfirstlane): as scalar-register values in the select chains of the caller they crash ROCm 7.2's greedy register allocator
    // (VirtRegAuxInfo::isRematerializable, iterative-ilp, the Nobs = 50 instantiation)
    int act_lo, act_hi, act_dyn;
};
__device__ __forceinline__ int opaque_i(int x) { asm("" : "+v"(x)); return x; }
// Is the windowed minimum `best` (squared) the global one?  With a2 = |p - p_ref|^2 and mo2 = the squared clearance of the window at
// p_ref, every segment outside the window is at least sqrt(mo2) - |p - p_ref| away from p (distances are 1-Lipschitz), so it is if
// sqrt(best) + |p - p_ref| < sqrt(mo2)  <=>  t = mo2 - a2 - best > 0 and t^2 > 4 a2 best.  The margins (1e-5 relative on squared
// distances) dwarf the rounding of the distance formula (<= 2e-10 relative wherever it matters; mo2 <= 1e-8 is stored as 0).
__device__ __forceinline__ bool window_is_global(double a2, double best, double mo2)
{
    const double t = mo2 - (a2 + best);
    return t > 1e-5 * mo2 && t * t > 4.0001 * (a2 * best);
}

// the circles of an instance whose edge lies within `radius` of the start position (bit k = circle k); padding slots (r = 0) never are
__device__ __forceinline__ unsigned long long circle_near_mask(const double *p, int N, int nobs, int lane, double radius)
{
    const double *ps = p + NZ + N;
    bool keep = false;
    if (lane < nobs) {
        const double dx = ps[3 * lane] - p[0], dy = ps[3 * lane + 1] - p[1], r = ps[3 * lane + 2], lim = radius + r;
        keep = r > 0.0 && fma(dx, dx, dy * dy) <= lim * lim;
    }
    return __ballot(keep);
}

// ---------------------------------------------------------------------------------------------
// psi(z; c, y), grad psi, F1 (av, aw), sum_k F2_k^2 (pen); WRITE_F2: F2_k also left in the LDS slice
// ---------------------------------------------------------------------------------------------
// CULL: `near` is the set of static circles that can be touched at all while every stage stays within KArgs.cull_radius of the start
// position (circle_near_mask below); the activity scan visits those only, and falls back to all of them for an evaluation in
// which some stage is farther away -- so the result is exactly that of the full scan.
// The handful of launch-uniform scalars an evaluation reads, as values of their own.  Read from the argument block (a.pb.*) they belong to a
// sixteen-dword scalar load whose registers the allocator spills and reloads AS ONE (sixteen v_readlane per use of one bound); a kernel that
// hands them over in this struct -- each passed through scalar_own() once -- pays two.
struct EvK { double ts, inv_ts, amin, amax, awmax; };
__device__ __forceinline__ double scalar_own(double x)
{
    // through a vector register and back (v_readfirstlane): a definition of its own that the coalescer cannot fold back into the loaded tuple
    int lo = __double2loint(x), hi = __double2hiint(x);
    asm volatile("" : "+v"(lo), "+v"(hi));
    return __hiloint2double(__builtin_amdgcn_readfirstlane(hi), __builtin_amdgcn_readfirstlane(lo));
}
__device__ __forceinline__ int scalar_own(int x)
{
    asm volatile("" : "+v"(x));
    return __builtin_amdgcn_readfirstlane(x);
}
// What the hybrid kernel's owner path hands over because its query points travel through LDS (nmpc_solve_hyb.h, "transport"): the control
// pair of the stage before (the last input for stage 0) -- read from the transport area one slot down instead of fetched from the neighbour
// lane --, this lane's slot of the area for handing (qa, qw) to the stage before, and the slot of the stage after (a zero pad behind the
// last stage).  Two pointers that the compiler cannot tell apart: the write stays in front of the read, and LDS serves a wave in order.
// Lanes 60..63 of such an evaluation hold zeros in zv, zw (Z60: group_prefix_ex_z60).
struct EvX {
    double vprev, wprev;
    lds_double2 *mine;
    const lds_double2 *next;
};
template <int P, class SH = ShapeAny, bool WRITE_F2 = false, bool CULL = false, int WIN = 0, bool Z60 = false>
__device__ __forceinline__ void eval_psi(const KArgs &a, lds_double *L, int f2off, int lane, int t, double zv, double zw,
                                         double c, double cbar_inv, double yv, double yw, double vref, const DynStage &dyn,
                                         bool want_grad, double &psi, double &pen_out, double &gv,
                                         double &gw, double &av_out, double &aw_out, unsigned long long near = ~0ull, WinState *ws = nullptr,
                                         ObsCert *oc = nullptr, long long *nmpc_pe = nullptr, const EvK *ek = nullptr, const EvX *evx = nullptr)
{
    static_assert(!Z60 || P == 20, "zero pads in lanes 60..63: the tri layout only");
    const int N = shape_N<SH>(a), nobs = shape_nobs<SH>(a), ndyn = shape_ndyn<SH>(a);
    const LdsMap mp = the_map<SH, P>(a);
    const double ts = ek ? ek->ts : a.pb.ts, inv_ts = ek ? ek->inv_ts : a.inv_ts;
    const double k_amin = ek ? ek->amin : a.pb.amin, k_amax = ek ? ek->amax : a.pb.amax, k_awmax = ek ? ek->awmax : a.pb.awmax;
    (void)nmpc_pe;
    // every stage lane of the tri layout is inside a 20-stage horizon; lanes 60..63 then hold
    // don't-care values that no cross-lane operation lets into the other lanes (nmpc_device.h)
    constexpr bool FULL = P == 20 && SH::N == 20;
    const bool in_r = t < N;                    // a real stage
    const bool in = FULL ? true : in_r;         // arithmetic masks: compile-time true when FULL
    const lds_double *sc = L + mp.sc;
    const double x0 = sc[SC_X0], y0 = sc[SC_Y0], th0 = sc[SC_TH0];
    const double xf = sc[SC_XF], yf = sc[SC_YF], thf = sc[SC_THF];

    // rollout (:88-90) as three prefix sums
    // (the pre-update state of a stage is the post-update state of the stage before: the same fma on the prefix sum of the stage before,
    // which the scan hands over with its own carry exchange -- group_prefix_ex)
    double ew_, ex_, ey_;
    auto prefix_ex = [lane](double v, double &excl) {
        if constexpr (Z60) return group_prefix_ex_z60(v, lane, excl);
        else return group_prefix_ex<P>(v, lane, excl);
    };
    const double thn = fma(ts, prefix_ex(zw, ew_), th0);
    const double th = t == 0 ? th0 : fma(ts, ew_, th0);
    double sn, cs;
    sincos_cw_t(th, (const lds_double *)(L + mp.cw), sn, cs);
    const double xn = fma(ts, prefix_ex(zv * cs, ex_), x0);
    const double yn = fma(ts, prefix_ex(zv * sn, ey_), y0);
    const double xp = t == 0 ? x0 : fma(ts, ex_, x0);
    const double yp = t == 0 ? y0 : fma(ts, ey_, y0);

    const double half_c = 0.5 * c;
    NMPC_EVTICK(nmpc_pe, 0);     // rollout

    double acc = (sc[SC_RV] * zv) * zv;                                           // (:84)
    acc = fma(sc[SC_RW] * zw, zw, acc);
    const double dv = zv - vref;                                                  // (:85)
    acc = fma(sc[SC_QV] * dv, dv, acc);
    {
        const double ddx = xp - xf, ddy = yp - yf, dth = th - thf;                // (:86, 59-64)
        acc = fma(sc[SC_Q], fma(ddx, ddx, ddy * ddy), acc);
        acc = fma(sc[SC_QTH] * dth, dth, acc);
    }
    // cross-track error: min over the N-1 reference segments (:121-144)
    double best = __builtin_inf();
    int bi = 0;
    bool full_scan = true;
    int i0c = 0;                        // first segment of the window the full scan measures the clearance of
    if constexpr (WIN > 0) {
        // WINDOWED SEARCH (exact).  From one evaluation to the next a stage's nearest segment rarely moves, so only the 2 WIN + 1
        // segments around the lane's window centre are measured -- per-lane LDS gathers instead of broadcasts -- and the result is
        // accepted if it is PROVABLY the full scan's (window_is_global above).  If any stage of the wave fails the test, or holds no
        // clearance yet, the full scan below runs instead and renews every lane's clearance; either way `best`, `bi` are the full scan's.
        const int nseg = N - 1;
        if (nseg >= 2 * WIN + 1) {
            int cc = ws->ctr;
            cc = cc < 0 ? 0 : (cc > nseg - 1 ? nseg - 1 : cc);
            i0c = cc - WIN;
            i0c = i0c < 0 ? 0 : (i0c > nseg - (2 * WIN + 1) ? nseg - (2 * WIN + 1) : i0c);
            if (!__any(in_r & !(ws->mo2 > 0.0))) {
                const lds_double *sg = L + mp.seg + SEG_STRIDE * i0c;
                double wv[2 * WIN + 1][5];
#pragma unroll
                for (int j = 0; j <= 2 * WIN; ++j)
#pragma unroll
                    for (int f = 0; f < 5; ++f) wv[j][f] = sg[j * SEG_STRIDE + f];
#pragma unroll
                for (int j = 0; j <= 2 * WIN; ++j) {
                    const double px = xn - wv[j][0], py = yn - wv[j][1];
                    const double dot = fma(px, wv[j][2], py * wv[j][3]);
                    const double that = dot * wv[j][4];
                    const double tst = fmin(fmax(that, 0.0), 1.0);
                    const double ex = fma(tst, wv[j][2], -px), ey = fma(tst, wv[j][3], -py);
                    const double d2 = fma(ex, ex, ey * ey);
                    bi = d2 < best ? i0c + j : bi;
                    best = fmin(best, d2);
                }
                const double ax = xn - ws->xr, ay = yn - ws->yr;
                const bool sure = window_is_global(fma(ax, ax, ay * ay), best, ws->mo2);
                full_scan = __any(in_r & !sure);
                NMPC_WIN_COUNT(0, full_scan);
                if (full_scan) {
                    // the full scan measures the clearance of the window around what the old window found nearest
                    i0c = bi - WIN;
                    i0c = i0c < 0 ? 0 : (i0c > nseg - (2 * WIN + 1) ? nseg - (2 * WIN + 1) : i0c);
                    best = __builtin_inf(); bi = 0;
                }
            }
        }
    }
    if (full_scan) {
        const lds_double *sg = L + mp.seg;
        const int nseg4 = (N - 1 + 3) & ~3;
        // software pipeline: the ten LDS reads of the NEXT pair of segments are issued before the current
        // pair is reduced (the scheduling barriers keep the compiler from sinking them to their uses)
        double cur[2][5], nxt[2][5];
        double mout = __builtin_inf();                      // (WIN) nearest segment outside the window [i0c, i0c + 2 WIN]
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int f = 0; f < 5; ++f) cur[j][f] = sg[j * SEG_STRIDE + f];
#pragma unroll SH::N > 0 ? (SH::N <= 20 ? 32 : 2) : 1
        for (int i = 0; i < nseg4; i += 2) {
            sg += 2 * SEG_STRIDE;                           // table is padded: reading one pair past the end is safe
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int f = 0; f < 5; ++f) nxt[j][f] = sg[j * SEG_STRIDE + f];
            NMPC_SCHED_BARRIER();
            double d2[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const double px = xn - cur[j][0], py = yn - cur[j][1];
                const double dot = fma(px, cur[j][2], py * cur[j][3]);
                const double that = dot * cur[j][4];
                const double tst = fmin(fmax(that, 0.0), 1.0);
                const double ex = fma(tst, cur[j][2], -px), ey = fma(tst, cur[j][3], -py);
                d2[j] = fma(ex, ex, ey * ey);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {                   // strict <: the first minimum keeps its index
                bi = d2[j] < best ? i + j : bi;
                best = fmin(best, d2[j]);
                if constexpr (WIN > 0) {                    // (a padding entry repeats the last segment)
                    const int ie = i + j < N - 1 ? i + j : N - 2;
                    mout = (unsigned)(ie - i0c) <= 2u * WIN ? mout : fmin(mout, d2[j]);
                }
            }
            NMPC_SCHED_BARRIER();
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int f = 0; f < 5; ++f) cur[j][f] = nxt[j][f];
        }
        if constexpr (WIN > 0) {
            // this lane's certificate for the evaluations to come: if the nearest segment lies in the window that was measured, the
            // window stays and its clearance is known; if not, the window moves there and the next evaluation measures it
            const bool inw = (unsigned)(bi - i0c) <= 2u * WIN;
            ws->ctr = inw ? i0c + WIN : bi;
            ws->xr = xn; ws->yr = yn;
            ws->mo2 = inw && mout > 1e-8 ? mout : 0.0;
        }
    }
    NMPC_EVTICK(nmpc_pe, 1);     // stage cost + CTE loop
    acc = fma(sc[SC_QCTE], best, acc);                                            // (:144)
    // accelerations (:160-161), their cost (:170-171) and the ALM term
    const double vprev = evx ? evx->vprev : from_prev<P>(zv, lane, sc[SC_VINIT]);
    const double wprev = evx ? evx->wprev : from_prev<P>(zw, lane, sc[SC_WINIT]);
    double av = (zv - vprev) * inv_ts, aw = (zw - wprev) * inv_ts;
    acc = fma(sc[SC_PA] * av, av, acc);
    acc = fma(sc[SC_PW] * aw, aw, acc);
    const double tv = fma(yv, cbar_inv, av), tw = fma(yw, cbar_inv, aw);
    double sv = tv - clampd(tv, k_amin, k_amax);
    double sw = tw - clampd(tw, -k_awmax, k_awmax);
    acc = fma(half_c, fma(sv, sv, sw * sw), acc);
    if (t == N - 1) {                                                             // terminal (:148)
        const double tx = xn - xf, ty = yn - yf, tth = thn - thf;
        acc = fma(sc[SC_QN], fma(tx, tx, ty * ty), acc);
        acc = fma(sc[SC_QTHN] * tth, tth, acc);
    }
    if (!in) { acc = 0.0; av = aw = sv = sw = 0.0; }
    av_out = av;
    aw_out = aw;
    const double fsum = group_sum<P>(acc, lane);
    NMPC_EVTICK(nmpc_pe, 2);     // accelerations, ALM term, cost sum

    // obstacle penalties on the post-update state (:106-119).  F2_k = sum_t max(0, h_kt); an obstacle that no stage
    // of any query point in this wave is inside of contributes exactly 0 to psi and to grad psi and is skipped
    // (wave-uniform branch).  The adjoint terms of a touched obstacle, c F2_k dh_kt/d(x, y), are added right where
    // its F2_k has just been summed -- same operations in the same order as a separate sweep would do them (cross-
    // track term first, circles in ascending order, then ellipses), without the round trip of F2 through LDS.
    double pen = 0.0;
    unsigned long long act = 0ull;      // wave-uniform: circles some stage is inside of
    unsigned act_dyn = 0u;              // wave-uniform: ellipses some stage is inside of
    bool scan = true;
    if (oc) {
        const double ox = xn - oc->xo, oy = yn - oc->yo;
        const bool sure = fma(ox, ox, oy * oy) < oc->m2;
        if (!__any(in_r & !sure)) {
            act = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(oc->act_hi) << 32) | (unsigned)__builtin_amdgcn_readfirstlane(oc->act_lo);
            act_dyn = (unsigned)__builtin_amdgcn_readfirstlane(oc->act_dyn);
            scan = false;
        }
        NMPC_WIN_COUNT(2, scan);
    }
    if (scan) {
        double mg = __builtin_inf();        // (oc) this lane's clearance from the obstacles the scan finds untouched
        const lds_double *ob = L + mp.obs;
        const int nobs4 = (nobs + 3) & ~3;
        if constexpr (CULL) {
            // only the circles of `near` -- unless a stage of this evaluation has left the radius the set was made for
            const unsigned long long all = nobs >= 64 ? ~0ull : (1ull << nobs) - 1ull;
            unsigned long long todo = near & all;
            if (todo != all) {
                const double rx = xn - x0, ry = yn - y0;
                const double rg = 0.999 * a.cull_radius;
                const double ro2 = fma(rx, rx, ry * ry);
                if (__any(in_r & !(ro2 <= rg * rg))) todo = all;
                else if (oc) mg = rg - __builtin_amdgcn_sqrt(ro2);      // the set holds while the stage stays inside the radius
            }
            while (todo) {                                  // four circles per trip; slot `nobs` holds an inert zero circle
                int kk[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    kk[j] = todo ? __builtin_ctzll(todo) : nobs;
                    todo &= todo - (todo ? 1ull : 0ull);
                }
                double od[16];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const lds_double *oj = ob + OBS_STRIDE * kk[j];
                    od[4 * j] = oj[0]; od[4 * j + 1] = oj[1]; od[4 * j + 2] = oj[2]; od[4 * j + 3] = oc ? oj[3] : 0.0;
                }
                NMPC_SCHED_BARRIER();
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double dx = xn - od[4 * j], dy = yn - od[4 * j + 1];
                    const double h = fma(-dy, dy, fma(-dx, dx, od[4 * j + 2]));       // (:112)
                    if (__any(in_r & (h > 0.0))) act |= 1ull << (kk[j] & 63);          // (the inert circle never is)
                    else if (oc) mg = fmin(mg, __builtin_amdgcn_sqrt(od[4 * j + 2] - h) - od[4 * j + 3]);
                }
            }
        } else {
#pragma unroll SH::NOBS >= 0 && SH::NOBS <= 16 ? 16 : 1
        for (int k = 0; k < nobs4; k += 4, ob += 4 * OBS_STRIDE) {      // activity scan: four circles per trip, one ballot each
            double od[16];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                od[4 * j] = ob[OBS_STRIDE * j]; od[4 * j + 1] = ob[OBS_STRIDE * j + 1]; od[4 * j + 2] = ob[OBS_STRIDE * j + 2];
                od[4 * j + 3] = oc ? ob[OBS_STRIDE * j + 3] : 0.0;
            }
            NMPC_SCHED_BARRIER();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double dx = xn - od[4 * j], dy = yn - od[4 * j + 1];
                const double h = fma(-dy, dy, fma(-dx, dx, od[4 * j + 2]));       // (:112)
                if (__any(in_r & (h > 0.0))) act |= 1ull << (k + j);
                else if (oc) mg = fmin(mg, __builtin_amdgcn_sqrt(od[4 * j + 2] - h) - od[4 * j + 3]);
            }
        }
        }
        NMPC_EVTICK(nmpc_pe, 5);     // static circle scan
        {
            double dv_[NDYN_MAX][DY_FIELDS];
#pragma unroll
            for (int k = 0; k < NDYN_MAX; ++k)
#pragma unroll
                for (int f = 0; f < DY_FIELDS; ++f) dv_[k][f] = k < ndyn ? dyn.get(k, f) : 0.0;
            NMPC_SCHED_BARRIER();
#pragma unroll
            for (int k = 0; k < NDYN_MAX; ++k) {
                if (k < ndyn) {
                    const double ca = dv_[k][DY_CA], sa = dv_[k][DY_SA];
                    const double dx = xn - dv_[k][DY_EX], dy = yn - dv_[k][DY_EY];
                    const double ea = fma(dx, ca, dy * sa);
                    const double eb = fma(dx, sa, -(dy * ca));
                    const double h = fma(-(eb * eb), dv_[k][DY_IRY2], fma(-(ea * ea), dv_[k][DY_IRX2], 1.0));   // (:118)
                    if (__any(in_r & (h > 0.0))) act_dyn |= 1u << k;
                    else if (oc)      // the ellipse lies inside the disc of its larger half axis
                        mg = fmin(mg, __builtin_amdgcn_sqrt(fma(dx, dx, dy * dy)) - __builtin_amdgcn_rsq(fmin(dv_[k][DY_IRX2], dv_[k][DY_IRY2])));
                }
            }
        }
        if (oc) {
            const double m = fma(0.99, mg, -1e-6);
            oc->xo = xn; oc->yo = yn;
            oc->m2 = m > 0.0 ? (m < 1e100 ? m * m : 1e200) : 0.0;
            oc->act_lo = opaque_i((int)(unsigned)act); oc->act_hi = opaque_i((int)(unsigned)(act >> 32)); oc->act_dyn = opaque_i((int)act_dyn);
        }
        NMPC_EVTICK(nmpc_pe, 6);     // ellipse scan
    }
    // ---- adjoint, first term: the cross-track error through the arg-min segment of this stage ----
    double gx = 0.0, gy = 0.0;
    if (want_grad) {
        const lds_double *sg = L + mp.seg + SEG_STRIDE * bi;
        const double px = xn - sg[0], py = yn - sg[1];
        const double dot = fma(px, sg[2], py * sg[3]);
        const double that = dot * sg[4];
        const double tst = fmin(fmax(that, 0.0), 1.0);
        const double ex = fma(tst, sg[2], -px), ey = fma(tst, sg[3], -py);
        const double ed = fma(ex, sg[2], ey * sg[3]);
        const double m = (that > 0.0 && that < 1.0) ? ed * sg[4] : 0.0;
        const double two_q = 2.0 * sc[SC_QCTE];
        gx = two_q * fma(m, sg[2], -ex);
        gy = two_q * fma(m, sg[3], -ey);
    }
    // ---- touched obstacles: F2_k, its square into the penalty, its adjoint terms ----
    if ((act | act_dyn) != 0ull) {
        for (unsigned long long rem = act; rem;) {          // two touched circles per trip: their tree sums interleave
            const int k0 = __builtin_ctzll(rem);
            rem &= rem - 1;
            if (rem == 0ull) {
                // a single circle left (the usual case of an instance that grazes an obstacle): one sum, not a pair with a dummy twin
                const lds_double *o0 = L + mp.obs + OBS_STRIDE * k0;
                const double ax = o0[0], ay = o0[1], ar = o0[2];
                const double dx0 = xn - ax, dy0 = yn - ay;
                const double h0 = fma(-dy0, dy0, fma(-dx0, dx0, ar));
                const double f20 = group_sum<P>(in ? fmax(h0, 0.0) : 0.0, lane);
                if (WRITE_F2 && t == 0) L[f2off + k0] = f20;
                pen = fma(f20, f20, pen);
                if (want_grad) {
                    const double w0 = -2.0 * (c * f20);
                    if (h0 > 0.0) { gx = fma(w0, dx0, gx); gy = fma(w0, dy0, gy); }
                }
                break;
            }
            const int k1 = __builtin_ctzll(rem);
            rem &= rem - 1;
            const lds_double *o0 = L + mp.obs + OBS_STRIDE * k0, *o1 = L + mp.obs + OBS_STRIDE * k1;
            const double ax = o0[0], ay = o0[1], ar = o0[2], bx = o1[0], by = o1[1], br = o1[2];
            const double dx0 = xn - ax, dy0 = yn - ay, dx1 = xn - bx, dy1 = yn - by;
            const double h0 = fma(-dy0, dy0, fma(-dx0, dx0, ar)), h1 = fma(-dy1, dy1, fma(-dx1, dx1, br));
            const double f20 = group_sum<P>(in ? fmax(h0, 0.0) : 0.0, lane);
            const double f21 = group_sum<P>(in ? fmax(h1, 0.0) : 0.0, lane);
            if (WRITE_F2 && t == 0) { L[f2off + k0] = f20; L[f2off + k1] = f21; }
            pen = fma(f20, f20, pen);
            pen = fma(f21, f21, pen);
            if (want_grad) {
                const double w0 = -2.0 * (c * f20), w1 = -2.0 * (c * f21);
                if (h0 > 0.0) { gx = fma(w0, dx0, gx); gy = fma(w0, dy0, gy); }
                if (h1 > 0.0) { gx = fma(w1, dx1, gx); gy = fma(w1, dy1, gy); }
            }
        }
#pragma unroll
        for (int k = 0; k < NDYN_MAX; ++k) {
            if (act_dyn & (1u << k)) {
                const double ca = dyn.get(k, DY_CA), sa = dyn.get(k, DY_SA);
                const double irx2 = dyn.get(k, DY_IRX2), iry2 = dyn.get(k, DY_IRY2);
                const double dx = xn - dyn.get(k, DY_EX), dy = yn - dyn.get(k, DY_EY);
                const double ea = fma(dx, ca, dy * sa);
                const double eb = fma(dx, sa, -(dy * ca));
                const double h = fma(-(eb * eb), iry2, fma(-(ea * ea), irx2, 1.0));      // (:118)
                const double f2 = group_sum<P>(in ? fmax(h, 0.0) : 0.0, lane);
                if (WRITE_F2 && t == 0) L[f2off + nobs + k] = f2;
                pen = fma(f2, f2, pen);
                if (want_grad) {
                    const double wk = -2.0 * (c * f2);
                    if (h > 0.0) {
                        const double A = ea * irx2, Bq = eb * iry2;
                        const double hx = fma(A, ca, Bq * sa);
                        const double hy = fma(A, sa, -(Bq * ca));
                        gx = fma(wk, hx, gx);
                        gy = fma(wk, hy, gy);
                    }
                }
            }
        }
    }
    psi = fma(half_c, pen, fsum);
    pen_out = pen;
    NMPC_EVTICK(nmpc_pe, 3);     // obstacles
    if (!want_grad) return;

    // ---- adjoint sweep, continued (what CasADi reverse AD generated for the reference) ----
    // the post-update state of stage t is the tracked state of stage t+1 (:86) or the terminal state (:148)
    const double wq = t < N - 1 ? sc[SC_Q] : sc[SC_QN];
    const double wth = t < N - 1 ? sc[SC_QTH] : sc[SC_QTHN];
    gx = fma(2.0 * wq, xn - xf, gx);
    gy = fma(2.0 * wq, yn - yf, gy);
    double gt = (2.0 * wth) * (thn - thf);
    double qa = fma(c, sv, (2.0 * sc[SC_PA]) * av);
    double qw = fma(c, sw, (2.0 * sc[SC_PW]) * aw);
    if (!in) { gx = gy = gt = qa = qw = 0.0; }
    const double Sx = group_suffix<P>(gx, lane);
    const double Sy = group_suffix<P>(gy, lane);
    const double e = fma(Sy, cs, -(Sx * sn));
    const double Dt = in ? (ts * zv) * e : 0.0;
    const double St = group_suffix<P>(in ? gt + from_next<P>(Dt, lane) : 0.0, lane);
    double qan, qwn;
    if (evx) { *evx->mine = dbl2{qa, qw}; const dbl2 n_ = *evx->next; qan = n_.x; qwn = n_.y; }
    else { qan = from_next<P>(qa, lane); qwn = from_next<P>(qw, lane); }
    const double dynv = fma(Sx, cs, Sy * sn);
    double g1 = fma(2.0 * sc[SC_RV], zv, (2.0 * sc[SC_QV]) * dv);
    g1 = fma(inv_ts, qa - qan, g1);
    g1 = fma(ts, dynv, g1);
    double g2 = (2.0 * sc[SC_RW]) * zw;
    g2 = fma(inv_ts, qw - qwn, g2);
    g2 = fma(ts, St, g2);
    gv = in ? g1 : 0.0;
    gw = in ? g2 : 0.0;
    NMPC_EVTICK(nmpc_pe, 4);     // adjoint sweep
}

// dot product of two horizon vectors (lane t holds the (v_t, w_t) pair)
template <int P>
__device__ __forceinline__ double hdot(double av, double aw, double bv, double bw, int lane)
{
    return group_sum<P>(fma(av, bv, aw * bw), lane);
}

// ---------------------------------------------------------------------------------------------
// cost-layer kernel: one evaluation per instance (parity tests, F1/F2 mapping API)
// ---------------------------------------------------------------------------------------------
template <int P>
__global__ __launch_bounds__(64) void nmpc_eval_kernel(KArgs a)
{
    extern __shared__ double lds[];
    constexpr int K = 64 / P;
    const int lane = threadIdx.x, g = lay_group<P>(lane), t = lay_stage<P>(lane);
    lds_double *L = (lds_double *)lds + g * a.map.total;
    const int N = a.pb.N;
    const bool in = t < N;
    const int inst = blockIdx.x * K + g;
    const int b = inst < a.B ? inst : a.B - 1;          // surplus groups redo the last instance, write nothing
    double vref;
    DynStage dyn;
    prepare_instance<P>(a, L, a.p + (size_t)b * a.n_p, t, vref, dyn);
    const double *u = a.u + (size_t)b * a.n_u;
    const double zv = in ? u[2 * t] : 0.0, zw = in ? u[2 * t + 1] : 0.0;
    const double c = a.ev_c ? a.ev_c[b] : 0.0;
    const double yv = (a.ev_y && in) ? a.ev_y[(size_t)b * a.n1 + t] : 0.0;
    const double yw = (a.ev_y && in) ? a.ev_y[(size_t)b * a.n1 + N + t] : 0.0;
    for (int k = t; k < a.n2; k += P) L[a.map.f2 + k] = 0.0;
    NMPC_WAVE_SYNC();
    double psi, pen, gv, gw, av, aw;
    eval_psi<P, ShapeAny, true>(a, L, a.map.f2, lane, t, zv, zw, c, 1.0 / fmax(c, 1.0), yv, yw, vref, dyn, true, psi, pen, gv, gw, av, aw);
    NMPC_WAVE_SYNC();          // F2_k written by lane 0 of the group are read by all its lanes below
    if (inst >= a.B) return;
    if (t == 0 && a.ev_psi) a.ev_psi[b] = psi;
    if (in) {
        if (a.ev_grad) { a.ev_grad[(size_t)b * a.n_u + 2 * t] = gv; a.ev_grad[(size_t)b * a.n_u + 2 * t + 1] = gw; }
        if (a.ev_F1) { a.ev_F1[(size_t)b * a.n1 + t] = av; a.ev_F1[(size_t)b * a.n1 + N + t] = aw; }
    }
    if (a.ev_F2) for (int k = t; k < a.n2; k += P) a.ev_F2[(size_t)b * a.n2 + k] = L[a.map.f2 + k];
}

}  // namespace nmpc

// nmpc_geom.h -- the loop's geometry that needs nothing of the device: the closest point on a segment, the cell of a coordinate, the
// rule for a grid axis and the fold of a position into a box.  The same operations in the same order on the host and on the device
// (the library is built without contraction), so that the kernels of nmpc_loop.h, the setter's WallGridHost::build and the mirror
// (trajectory.segment_closest / grid_cellof / grid_axis) agree bit for bit.  tests/loop_geometry_main.cpp compiles it for the host.
// Nothing is included: the builtins below exist in hipcc's device code and in g++ alike.
#pragma once

#ifdef __HIPCC__
#define NMPC_GEOM_FN __host__ __device__ inline
#else
#define NMPC_GEOM_FN inline
#endif

namespace nmpc {

// The point (cx, cy) of the segment (x1, y1) -> (x2, y2) closest to (x, y), -> the squared distance to it.  Unfused f64 in the order
// written, no sqrt.  A segment without length (L2 == 0, by coincident ends or by underflow) is its first end; a comparison that is
// false (a NaN) clamps nothing.  clamp_below = false lets the segment run on backwards beyond its first end (segment 0 of a route:
// nmpc_loop_track_kernel); every other caller passes true.
NMPC_GEOM_FN double segment_closest(double x, double y, double x1, double y1, double x2, double y2, bool clamp_below, double &cx, double &cy)
{
    const double ex = x2 - x1, ey = y2 - y1;
    const double L2 = ex * ex + ey * ey;
    double t = 0.0;
    if (L2 > 0.0) {
        t = ((x - x1) * ex + (y - y1) * ey) / L2;
        if (t < 0.0 && clamp_below) t = 0.0;
        if (t > 1.0) t = 1.0;
    }
    cx = x1 + t * ex; cy = y1 + t * ey;
    const double dx = x - cx, dy = y - cy;
    return dx * dx + dy * dy;
}

// the cell of coordinate v on an axis of n cells of edge h from o: monotone non-decreasing in v (every operation is; t is a NaN only
// with a NaN v or with h = inf, where every v answers 0), clamped in double before the conversion.  Filing and looking up, in both
// grids, use this one function.
NMPC_GEOM_FN int cellof(double v, double o, double h, int n)
{
    const double t = (v - o) / h;
    if (!(t > 0.0)) return 0;
    if (t >= (double)n) return n - 1;
    return (int)t;
}

// an axis of a grid: cells of edge `cell` over the extent >= 0, or `cap` cells of edge extent / cap where that would be more
NMPC_GEOM_FN void grid_axis(double extent, double cell, int cap, int &n, double &h)
{
    const double q = extent / cell;
    if (q < (double)cap) { n = (int)q + 1; h = cell; }
    else { n = cap; h = extent / (double)cap; }
}

// (x, y) into the box (lx, ly) .. (hx, hy) of the finite positions: a stage with a NaN or an infinity is in nobody's D and in no box
NMPC_GEOM_FN void box_fold(double x, double y, double &lx, double &ly, double &hx, double &hy)
{
    const double inf = __builtin_inf();
    if (__builtin_fabs(x) < inf && __builtin_fabs(y) < inf) {
        lx = x < lx ? x : lx; ly = y < ly ? y : ly;
        hx = x > hx ? x : hx; hy = y > hy ? y : hy;
    }
}

}  // namespace nmpc

// The loop's geometry (csrc/nmpc_geom.h) compiled for the host.  argv[1] names a file of cases, one per line, doubles in any form
// strtod reads (hexadecimal, inf, nan):
//   S x y x1 y1 x2 y2 clamp_below   -> S <bits of v> <bits of cx> <bits of cy>     segment_closest
//   C v o h n                       -> C <cell>                                    cellof
//   A extent cell cap               -> A <n> <bits of h>                           grid_axis
//   B k  x_0 y_0 ... x_k-1 y_k-1    -> B <bits of lx ly hx hy>                     box_fold over the k positions, from (inf, inf, -inf, -inf)
// tests/test_loop_geometry.py compares the lines with the NumPy mirror's.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "nmpc_geom.h"

static uint64_t bits(double v)
{
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string kind, w;
        ss >> kind;
        double a[7];
        int n = 0;
        auto num = [&]() { ss >> w; return std::strtod(w.c_str(), nullptr); };
        if (kind == "S") {
            for (double &v : a) v = num();
            double cx, cy;
            const double v = nmpc::segment_closest(a[0], a[1], a[2], a[3], a[4], a[5], a[6] != 0.0, cx, cy);
            std::printf("S %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits(v), bits(cx), bits(cy));
        } else if (kind == "C") {
            for (int i = 0; i < 3; ++i) a[i] = num();
            ss >> n;
            std::printf("C %d\n", nmpc::cellof(a[0], a[1], a[2], n));
        } else if (kind == "A") {
            for (int i = 0; i < 2; ++i) a[i] = num();
            int cap = 0;
            ss >> cap;
            double h = 0.0;
            nmpc::grid_axis(a[0], a[1], cap, n, h);
            std::printf("A %d %016" PRIx64 "\n", n, bits(h));
        } else if (kind == "B") {
            ss >> n;
            double lx = __builtin_inf(), ly = lx, hx = -lx, hy = -lx;
            for (int i = 0; i < n; ++i) {
                const double x = num(), y = num();
                nmpc::box_fold(x, y, lx, ly, hx, hy);
            }
            std::printf("B %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits(lx), bits(ly), bits(hx), bits(hy));
        } else {
            return 3;
        }
    }
    return 0;
}

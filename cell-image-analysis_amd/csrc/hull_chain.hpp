// hull_chain.hpp -- the convex hull of an object's pixel-edge midpoints as ex_region_pass (extract.hip) and sh_outline (shape.hip)
// build it: two monotone chains over the row extremes in LDS, in doubled coordinates of the object's bounding-box window (row i,
// column j: y = 2i, x = 2j, the midpoints at (2i +- 1, 2j) and (2i, 2j +- 1)), and the exact integer helpers that count the pixel
// centres inside or on it.  rowL / rowR hold each row's first and last column of the object, 0x7fff and -1 for a row without one.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

namespace cs {

__device__ inline long long floor_div(long long a, long long d) { return a >= 0 ? a / d : -((-a + d - 1) / d); }   // d > 0
__device__ inline long long ceil_div(long long a, long long d) { return -floor_div(-a, d); }

__device__ inline int pack_pt(int y, int x) { return ((y + 1) << 16) | (x + 1); }
__device__ inline int pt_y(int p) { return (p >> 16) - 1; }
__device__ inline int pt_x(int p) { return (p & 0xffff) - 1; }

// Andrew's monotone chain over the left (right) extreme points in increasing y: the convex minorant (concave majorant) of x(y)
__device__ inline int build_chain(const short* rowE, int h, bool right, int* ch)
{
    int k = 0;
    for (int t = 0; t <= 2 * h; ++t) {
        const int y = t - 1;
        int x;
        bool have = false;
        if ((y & 1) == 0) {
            const int e = rowE[y >> 1];
            if (right ? e >= 0 : e < 0x7fff) { x = right ? 2 * e + 1 : 2 * e - 1; have = true; }
        } else {
            const int i0 = (y - 1) >> 1, i1 = i0 + 1;                     // rows above and below the odd line
            x = right ? INT_MIN : INT_MAX;
            if (i0 >= 0) {
                const int e = rowE[i0];
                if (right ? e >= 0 : e < 0x7fff) { x = right ? max(x, 2 * e) : min(x, 2 * e); have = true; }
            }
            if (i1 < h) {
                const int e = rowE[i1];
                if (right ? e >= 0 : e < 0x7fff) { x = right ? max(x, 2 * e) : min(x, 2 * e); have = true; }
            }
        }
        if (!have) continue;
        while (k >= 2) {
            const int o = ch[k - 2], a = ch[k - 1];
            const long long cr = (long long)(pt_y(a) - pt_y(o)) * (long long)(x - pt_x(o)) -
                                 (long long)(pt_x(a) - pt_x(o)) * (long long)(y - pt_y(o));
            if (right ? cr >= 0 : cr <= 0) --k; else break;
        }
        ch[k++] = pack_pt(y, x);
    }
    return k;
}

// the chain's segment that holds y (chain sorted by y, y within its range): largest k <= n-2 with y_k <= y
__device__ inline int chain_segment(const int* ch, int n, int y)
{
    int lo = 0, hi = n - 2;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pt_y(ch[mid]) <= y) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace cs

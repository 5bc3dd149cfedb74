// Row-mapped indexing of the element-wise kernels (ew_kernels.hip, the checkerboard kernels of entropy.hip).
#pragma once
#include "common.h"

#define EW_BLOCK 256

// ------------------------------------------------------------------------------------------------
// Row-mapped indexing (round 6).  The grid-stride form below every kernel of this file started with -- a 64-bit linear index
// taken apart by three 64-bit divisions per element -- costs ~300 vector instructions per element, more than the element's own
// work (k_axpby, one float per thread, was 4.8 % of the configs[4] frame).  ROWS: blockIdx.z = image, blockIdx.y (+ a grid stride) = row,
// the threads of blockIdx.x walk the w * per_px work items of the row; item -> (x, c) by ONE multiply-high with a host-made reciprocal
// (exact while item * per_px < 2^32; vc_rowmap_make checks it).  The linear form stays as the fallback for shapes outside that.
// The body of a kernel is the same lambda under both forms: same arithmetic per element, same bits.
// ------------------------------------------------------------------------------------------------
struct vc_rowmap {
    unsigned items, per_px, magic;
};

static inline bool vc_rowmap_make(vc_rowmap &m, int n, int h, int w, int per_px)
{
    if (n < 1 || h < 1 || w < 1 || per_px < 1 || n > 65535 || h > 65535) return false;
    const unsigned long long items = (unsigned long long)w * (unsigned long long)per_px;
    if (items >= (1ull << 24) || items * (unsigned long long)per_px >= (1ull << 32)) return false;
    m.items = (unsigned)items;
    m.per_px = (unsigned)per_px;
    m.magic = per_px == 1 ? 0u : (unsigned)((1ull << 32) / (unsigned long long)per_px) + 1u;
    return true;
}

template <bool ROWS, class F>
__device__ __forceinline__ void ew_for_each(const vc_rowmap &m, int N, int H, int W, int PP, F f)
{
    if constexpr (ROWS) {
        const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
        if (j >= m.items) return;
        const unsigned x = m.per_px == 1 ? j : __umulhi(j, m.magic);
        const int c = (int)(j - __umul24(x, m.per_px));
        for (int y = blockIdx.y; y < H; y += gridDim.y) f((int)blockIdx.z, y, (int)x, c);      // (x, c) once per thread, rows in a grid stride
    } else {
        const long long total = (long long)N * H * W * PP;
        for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
            const int c = (int)(i % PP);
            long long t = i / PP;
            const int x = (int)(t % W); t /= W;
            const int y = (int)(t % H);
            const int n = (int)(t / H);
            f(n, y, x, c);
        }
    }
}

// grid of the row form: enough rows per grid step that ~8192 workgroups exist (a workgroup per row of a big tensor would be 65 K
// workgroups of one element per thread: measured slower than the grid-stride form on the pooling kernel), the rest in the row loop
static inline dim3 vc_rowmap_grid(const vc_rowmap &m, int n, int h)
{
    const long long bx = (m.items + EW_BLOCK - 1) / EW_BLOCK;
    long long gy = (8192 + bx * n - 1) / (bx * n);
    if (gy < 1) gy = 1;
    if (gy > h) gy = h;
    return dim3((unsigned)bx, (unsigned)gy, (unsigned)n);
}

// launch `rows` (the ROWS = true instance) on the row grid when the shape allows it, `lin` (ROWS = false) on the grid-stride grid otherwise
#define VC_EW_LAUNCH(st, KERN, N, H, W, PP, ...)                                                                                   \
    do {                                                                                                                           \
        vc_rowmap m_;                                                                                                              \
        if (vc_rowmap_make(m_, (N), (H), (W), (PP)))                                                                               \
            KERN<true><<<vc_rowmap_grid(m_, (N), (H)), dim3(EW_BLOCK), 0, (st)>>>(__VA_ARGS__, m_);                                \
        else                                                                                                                       \
            KERN<false><<<dim3(ew_grid((long long)(N) * (H) * (W) * (PP), EW_BLOCK)), dim3(EW_BLOCK), 0, (st)>>>(__VA_ARGS__, vc_rowmap{0, 0, 0}); \
    } while (0)

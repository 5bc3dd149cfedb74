// Modulated deformable 3x3 convolution (torchvision.ops.deform_conv2d semantics) for the ICIP2024 OffsetDiversity
// fusion (ICIP2024/src/model/helpers.py:35-58).  Gather-bound, not matrix-bound: per output pixel and group the
// kernel samples 9 taps x 4 corners x cg channels (cg = 8..16 contiguous values) and contracts them with
// 9*cg*og weights; one lane owns one (pixel, group) pair and the group index is uniform per wave
// (the vector path reads the weights through the scalar cache, the scalar path from LDS).  The offset/mask preparation of OffsetDiversity.prep (tanh *
// magnitude + flipped flow, sigmoid) is folded into the offset fetch in the fused entry point.
#include "common.h"

namespace {

struct DeformArgs {
    vc_view x1, x2;        // inputs of the first / second half of the groups (generic mode: x2 == x1 shifted)
    vc_view off1, off2;    // generic: offset tensor halves;   fused: raw offset-net outputs (27 * G/2 channels)
    vc_view msk1, msk2;    // generic: mask halves (p may be 0); fused: unused
    vc_view flow1, flow2;  // fused only
    vc_view out;
    const float *wpk, *bias;
    float magnitude;
    int groups;
    int x_half;            // fp16 path: x1 / x2 point at half-precision features (strides in elements); 2: group-planar ones
    int twl;               // log2 of the pixel tile's width: a wave's 64 lanes are a (64 >> twl) x (1 << twl) tile
    unsigned gstride;      // vector path: bytes from one group's channels to the next one's (cg * element size; planar: h * w * cg * 2)
};

// Branch-free tanh / logistic for the half-precision vector path: the library's tanhf spelled out (its polynomial below 0.625,
// 1 - 2 / (e^2|x| + 1) with the library's expf and the hardware reciprocal above) as ONE straight-line sequence with a select
// instead of two branch sides that a divergent wave both runs -- the same bits as tanhf, which the fp32 instances call; the
// logistic is their expression too.  (tests/test_icip2024_gpu.py holds the two instances together at 1e-6.)
__device__ __forceinline__ float tanh_bf(float x)
{
    const float ax = fabsf(x), x2 = x * x;
    const float big = fmaf(__builtin_amdgcn_rcpf(expf(2.0f * ax) + 1.0f), -2.0f, 1.0f);   // e^(2|x|) = +inf for large |x| -> 1
    float p = fmaf(x2, -0x1.758e7ap-8f, 0x1.521192p-6f);
    p = fmaf(x2, p, -0x1.b8389cp-5f);
    p = fmaf(x2, p, 0x1.110704p-3f);
    p = fmaf(x2, p, -0x1.555532p-2f);
    const float small = fmaf(x2, ax * p, ax);
    return copysignf(ax < 0.625f ? small : big, x);                            // (NaN: the comparison is false, `big` is NaN)
}

__device__ __forceinline__ float sigmoid_bf(float x)
{
    return 1.0f / (1.0f + expf(-x));
}

// One workgroup = one 4 x 16 pixel tile (args.twl) x all G/2 groups of ONE reference (wave w <-> group w of that half): the
// waves of a workgroup then consume every channel of the 128-byte lines they pull in (a group alone uses only
// cg of the C channels of a pixel), and the per-pixel offset/mask record of that reference is read completely
// by the workgroup.  Lanes of a wave are the 64 pixels of the tile, so the group (and its weights) is wave-uniform.
// With pixel-interleaved features every lane of a gather meets its own 128-byte line (a pixel is C * 2 or C * 4 bytes);
// the fp16 path therefore gathers from GROUP-PLANAR half features (vc_to_half_planar, vc_offset_diversity_hxp: one group's
// cg halves of neighbouring pixels are neighbours in memory), 8-16 lines per gather when neighbouring pixels sample
// neighbouring positions: 3.21 -> 2.10 ms on the 128 -> 64 fusion @1088x1920 of the configs[4] frame, bit-identical results.
// MAXT: 512 when the half has at most 8 groups (the ICIP2024 model: 16 groups) -- leaves the register file for the batched
// gathers; 1024 (up to 16 groups per half) keeps 128 registers and gathers one tap at a time.
// MODE: how a tap's offset / modulation come about -- a compile-time property of the instance, nothing of it is decided in the tap loop.
//   MODE_GENERIC  offsets and (optional) mask are read as they lie in their tensors (vc_deform_conv2d)
//   MODE_OD       the raw record of OffsetDiversity: tanh * magnitude + flipped flow, logistic on the mask (vc_offset_diversity*)
//   MODE_PAIR     the raw record of two plain modulated layers (ICIP2023 DeformB.get_deformed_maps): offsets as they come, logistic
//                 on the mask, no flow (vc_deform_pair; vc_deform_pair_hxp: the XH body on group-planar half features)
// MODE_OD and MODE_PAIR share the record fetch (FUSED below).
enum { MODE_GENERIC = 0, MODE_OD = 1, MODE_PAIR = 2 };

template <int CG, int OG, int MODE, bool VEC, int RV = 1, int MAXT = 1024, bool XH = false>
__global__ void __launch_bounds__(MAXT) k_deform(DeformArgs a)
{
    constexpr bool FUSED = MODE != MODE_GENERIC;
    extern __shared__ float wsm_all[];
    const int half = a.groups / 2;
    const bool second = blockIdx.y != 0;
    const int n = blockIdx.z;
    const int nthreads = 64 * half;
    const float *wsrc = a.wpk + (long long)(second ? half : 0) * 9 * CG * OG;
    constexpr bool WLDS = !(VEC && XH);                // (the half-precision vector path reads its group's weights through the scalar cache)
    if constexpr (WLDS)
        for (int i = threadIdx.x; i < half * 9 * CG * OG; i += nthreads) wsm_all[i] = wsrc[i];
    const int gl = threadIdx.x >> 6;                  // group inside its half == wave index
    const int g = second ? gl + half : gl;
    const int lane = threadIdx.x & 63;
    const float *wsm = wsm_all + gl * 9 * CG * OG;
    const vc_view &X = second ? a.x2 : a.x1;
    const vc_view &O = second ? a.off2 : a.off1;
    const vc_view &M = second ? a.msk2 : a.msk1;
    const vc_view &FL = second ? a.flow2 : a.flow1;
    const int H = a.out.h, W = a.out.w;
    const int twl = a.twl, twm = (1 << twl) - 1;
    const int tiles_x = (W + twm) >> twl;
    const int ty0 = (blockIdx.x / tiles_x) * (64 >> twl), tx0 = (blockIdx.x % tiles_x) << twl;
    const int y = ty0 + (lane >> twl), x = tx0 + (lane & twm);
    // FUSED: the 27*half-float offset/mask record of each of the 64 pixels is fetched ONCE by the workgroup with
    // coalesced loads (a lane reading its own 18+9 values straight from global touches 27 separate 4-byte words
    // 1.7 KB apart from its neighbours': 1.4 of 3.2 ms at 544x960) and parked in LDS at an odd pixel stride.
    const int RS = 27 * half + 1;                      // record stride in floats (odd for half = 8: 217)
    float *rec = wsm_all + (WLDS ? half * 9 * CG * OG : 0);
    if (FUSED) {
        // `half` threads per pixel, thread s of a pixel takes the RV-float pieces s, s + half, ... of its record: a wave
        // instruction reads whole contiguous stretches (128 bytes per pixel for RV = 4, half = 8), and the (27 + RV - 1) / RV
        // loads of a thread are all issued before the first one is waited for.  (The first version walked the record
        // with one 4-byte load per thread and iteration, 27 dependent global round trips per workgroup: 54 us of its 60.)
        constexpr int IT = (27 + RV - 1) / RV;
        const int per_px = 27 * half, pieces = per_px / RV;           // per_px % RV == 0 (select_route)
        const int px = threadIdx.x / half, s = threadIdx.x - px * half;
        const int yy = min(ty0 + (px >> twl), H - 1), xx = min(tx0 + (px & twm), W - 1);
        const float *src = O.p + view_off(O, n, yy, xx);
        float v[IT][RV];
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            const int pc = min(s + j * half, pieces - 1);
            if constexpr (RV == 4) {
                const f32x4 t = *reinterpret_cast<const f32x4 *>(src + 4 * pc);
                v[j][0] = t.x, v[j][1] = t.y, v[j][2] = t.z, v[j][3] = t.w;
            } else if constexpr (RV == 2) {
                const float2 t = *reinterpret_cast<const float2 *>(src + 2 * pc);
                v[j][0] = t.x, v[j][1] = t.y;
            } else {
                v[j][0] = src[pc];
            }
        }
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            const int pc = s + j * half;
            if (pc < pieces) {
#pragma unroll
                for (int e = 0; e < RV; ++e) rec[px * RS + RV * pc + e] = v[j][e];     // (odd record stride: scalar LDS writes)
            }
        }
    }
    __syncthreads();
    if (y >= H || x >= W) return;

    float acc[OG];
#pragma unroll
    for (int o = 0; o < OG; ++o) acc[o] = a.bias ? a.bias[g * OG + o] : 0.0f;

    const float *op = FUSED ? rec + lane * RS + gl * 18 : O.p + view_off(O, n, y, x) + gl * 18;
    const float *mp = FUSED ? rec + lane * RS + half * 18 + gl * 9
                            : (M.p ? M.p + view_off(M, n, y, x) + gl * 9 : nullptr);
    float fu = 0.0f, fv = 0.0f;
    if (MODE == MODE_OD) {
        const float *fp = FL.p + view_off(FL, n, y, x);
        fu = fp[0];
        fv = fp[1];
    }
    // (XH: half-precision features -- a group's CG channels of a pixel are CG / 8 gathers of 16 bytes instead of CG / 4; the
    //  kernel is bound by the gathers, every lane of an instruction in a different 128-byte line, so that halves it)
    constexpr int ESZ = XH ? 2 : 4;
    const unsigned char *xbase = reinterpret_cast<const unsigned char *>(X.p) + ((long long)n * X.sn + gl * CG) * ESZ;

    // One tap's sampling geometry.  Nothing below sits under a branch: a corner (or a whole tap) outside the image gets
    // its address clamped into the image and its VALUE replaced by zero after the load, so the 4 * CG / 4 gathers of all
    // taps of a batch are issued back to back and their L2 round trips overlap.  (With the loads under `if`s the compiler
    // waited for each of them in turn: ~45 dependent round trips per wave, 53 us per workgroup at 1088x1920.)
    struct Tap {
        const unsigned char *p1, *p2, *p3, *p4;
        float w1, w2, w3, w4, m;
        bool ok, tl, tr, bl, br;
    };
    auto tap = [&](int k) {
        Tap q;
        float dy = op[2 * k], dx = op[2 * k + 1];
        q.m = 1.0f;
        if (MODE == MODE_OD) {
            dy = tanhf(dy) * a.magnitude + fv;        // flow.flip(1): (v, u) pairs with (dy, dx)
            dx = tanhf(dx) * a.magnitude + fu;
            q.m = 1.0f / (1.0f + expf(-mp[k]));
        } else if (MODE == MODE_PAIR) {
            q.m = 1.0f / (1.0f + expf(-mp[k]));
        } else if (mp) {
            q.m = mp[k];
        }
        const float py = (float)(y - 1 + k / 3) + dy;
        const float px = (float)(x - 1 + k % 3) + dx;
        q.ok = py > -1.0f && py < (float)H && px > -1.0f && px < (float)W;      // also rejects NaN
        const float fy = floorf(py), fx = floorf(px);
        const int y0 = q.ok ? (int)fy : 0, x0 = q.ok ? (int)fx : 0, y1 = y0 + 1, x1 = x0 + 1;
        const float lh = py - fy, lw = px - fx, hh = 1.0f - lh, hw = 1.0f - lw;
        q.w1 = hh * hw, q.w2 = hh * lw, q.w3 = lh * hw, q.w4 = lh * lw;
        const bool t = y0 >= 0, b = y1 <= H - 1, l = x0 >= 0, r = x1 <= W - 1;
        q.tl = q.ok && t && l, q.tr = q.ok && t && r, q.bl = q.ok && b && l, q.br = q.ok && b && r;
        const long long r0 = (long long)max(y0, 0) * X.sh * ESZ, r1 = (long long)min(y1, H - 1) * X.sh * ESZ;
        const long long c0 = (long long)max(x0, 0) * X.sw * ESZ, c1 = (long long)min(x1, W - 1) * X.sw * ESZ;
        q.p1 = xbase + r0 + c0, q.p2 = xbase + r0 + c1, q.p3 = xbase + r1 + c0, q.p4 = xbase + r1 + c1;
        return q;
    };
    if constexpr (VEC && XH) {
        // Half-precision features (round 6).  The round-5 form of this path issued ~3 200 vector instructions per (pixel, group):
        // 12 of every 356 per tap quarter-rate 64-bit multiplies of the address arithmetic, ~95 the two library tanhf calls (both
        // sides of their branch run in a divergent wave).  Here ~1 700: 32-bit byte offsets from a wave-uniform base (24-bit
        // multiplies; the launcher refuses images above 4 GiB), branch-free tanh (the library's arithmetic, both sides computed,
        // one select), the out-of-image zeroing on the four bilinear weights instead of the gathered values, two channels per
        // packed-fp32 instruction, the group's weights through the scalar cache (wave-uniform: no LDS, no vector registers).
        // That alone bought 3 % (3.34 -> 3.22 ms, C = 64 @1088x1920): the kernel is bound by its gathers, by how many cache lines
        // each one meets -- what pays is the group-planar layout of the features (a.gstride; 3.22 -> 2.36 ms), and NOT more gathers
        // in flight: a fence that issues a whole batch before its first use costs 30 %.
#ifndef VC_DEFORM_TB
#define VC_DEFORM_TB 3
#endif
        constexpr int TB = (MAXT > 512 || CG > 8) ? 1 : VC_DEFORM_TB;       // taps per batch (divides 9; one tap per batch measured 5 % slower)
        constexpr int V = (CG + 7) / 8;                          // gathers per corner: 16 bytes each; CG % 8 == 4: the last one 8 bytes
        constexpr int EPV = 8;                                   // channels per gather
        constexpr bool TAIL8 = (CG % 8) == 4;
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        typedef _Float16 h8 __attribute__((ext_vector_type(8)));
        const unsigned char *xb = reinterpret_cast<const unsigned char *>(X.p) + (long long)n * X.sn * ESZ;      // wave-uniform
        const unsigned rowB = (unsigned)(X.sh * ESZ), pixB = (unsigned)(X.sw * ESZ), goff = (unsigned)gl * a.gstride;
        const int gu = __builtin_amdgcn_readfirstlane(g);
        const float *wg = a.wpk + (long long)gu * 9 * CG * OG;
        struct TapV {
            unsigned o1, o2, o3, o4;
            float w1, w2, w3, w4, m;
        };
        auto tapv = [&](int k) {
            TapV q;
            float dy = op[2 * k], dx = op[2 * k + 1], m = 1.0f;
            if (MODE == MODE_OD) {
                dy = fmaf(tanh_bf(dy), a.magnitude, fv);          // flow.flip(1): (v, u) pairs with (dy, dx)
                dx = fmaf(tanh_bf(dx), a.magnitude, fu);
                m = sigmoid_bf(mp[k]);
            } else if (MODE == MODE_PAIR) {
                m = sigmoid_bf(mp[k]);
            } else if (mp) {
                m = mp[k];
            }
            const float py = (float)(y - 1 + k / 3) + dy;
            const float px = (float)(x - 1 + k % 3) + dx;
            const bool ok = py > -1.0f && py < (float)H && px > -1.0f && px < (float)W;      // also rejects NaN
            const float fy = floorf(py), fx = floorf(px);
            const int y0 = ok ? (int)fy : 0, x0 = ok ? (int)fx : 0, y1 = y0 + 1, x1 = x0 + 1;
            const float lh = py - fy, lw = px - fx, hh = 1.0f - lh, hw = 1.0f - lw;
            const bool t = y0 >= 0, b = y1 <= H - 1, l = x0 >= 0, r = x1 <= W - 1;
            // (a corner -- or a whole tap -- outside the image: address clamped into the image, WEIGHT zero; a NaN position ends here too)
            q.w1 = (ok && t && l) ? hh * hw : 0.0f, q.w2 = (ok && t && r) ? hh * lw : 0.0f;
            q.w3 = (ok && b && l) ? lh * hw : 0.0f, q.w4 = (ok && b && r) ? lh * lw : 0.0f;
            q.m = m;
            const unsigned r0 = __umul24((unsigned)max(y0, 0), rowB) + goff, r1 = __umul24((unsigned)min(y1, H - 1), rowB) + goff;
            const unsigned c0 = __umul24((unsigned)max(x0, 0), pixB), c1 = __umul24((unsigned)min(x1, W - 1), pixB);
            q.o1 = r0 + c0, q.o2 = r0 + c1, q.o3 = r1 + c0, q.o4 = r1 + c1;
            return q;
        };
        f32x2 acc2[OG / 2];
#pragma unroll
        for (int o = 0; o < OG / 2; ++o) acc2[o] = f32x2{acc[2 * o], acc[2 * o + 1]};
#pragma unroll 1
        for (int k0 = 0; k0 < 9; k0 += TB) {     // (rolled: unrolled, the compiler hoists all 9 * CG * OG weight reads and spills)
            TapV q[TB];
            f32x4 v[TB][4][V];
#pragma unroll
            for (int j = 0; j < TB; ++j) {
                q[j] = tapv(k0 + j);
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    if (TAIL8 && c == V - 1) {
                        const float2 t1 = *reinterpret_cast<const float2 *>(xb + (size_t)(q[j].o1 + 16 * c)), t2 = *reinterpret_cast<const float2 *>(xb + (size_t)(q[j].o2 + 16 * c));
                        const float2 t3 = *reinterpret_cast<const float2 *>(xb + (size_t)(q[j].o3 + 16 * c)), t4 = *reinterpret_cast<const float2 *>(xb + (size_t)(q[j].o4 + 16 * c));
                        v[j][0][c] = f32x4{t1.x, t1.y, 0.f, 0.f}, v[j][1][c] = f32x4{t2.x, t2.y, 0.f, 0.f};
                        v[j][2][c] = f32x4{t3.x, t3.y, 0.f, 0.f}, v[j][3][c] = f32x4{t4.x, t4.y, 0.f, 0.f};
                    } else {
                        v[j][0][c] = *reinterpret_cast<const f32x4 *>(xb + (size_t)(q[j].o1 + 16 * c));
                        v[j][1][c] = *reinterpret_cast<const f32x4 *>(xb + (size_t)(q[j].o2 + 16 * c));
                        v[j][2][c] = *reinterpret_cast<const f32x4 *>(xb + (size_t)(q[j].o3 + 16 * c));
                        v[j][3][c] = *reinterpret_cast<const f32x4 *>(xb + (size_t)(q[j].o4 + 16 * c));
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < TB; ++j) {
                const float *wk = wg + (k0 + j) * CG * OG;
                const f32x2 w1 = {q[j].w1, q[j].w1}, w2 = {q[j].w2, q[j].w2}, w3 = {q[j].w3, q[j].w3}, w4 = {q[j].w4, q[j].w4}, mm = {q[j].m, q[j].m};
#pragma unroll
                for (int c = 0; c < V; ++c) {
#pragma unroll
                    for (int e = 0; e < ((TAIL8 && c == V - 1) ? 4 : EPV); e += 2) {
                        const h8 h1 = __builtin_bit_cast(h8, v[j][0][c]), h2 = __builtin_bit_cast(h8, v[j][1][c]);
                        const h8 h3 = __builtin_bit_cast(h8, v[j][2][c]), h4 = __builtin_bit_cast(h8, v[j][3][c]);
                        const f32x2 e1 = {(float)h1[e], (float)h1[e + 1]}, e2 = {(float)h2[e], (float)h2[e + 1]};
                        const f32x2 e3 = {(float)h3[e], (float)h3[e + 1]}, e4 = {(float)h4[e], (float)h4[e + 1]};
                        f32x2 val = e1 * w1;
                        val = __builtin_elementwise_fma(e2, w2, val);
                        val = __builtin_elementwise_fma(e3, w3, val);
                        val = __builtin_elementwise_fma(e4, w4, val) * mm;
                        const float *wc = wk + (EPV * c + e) * OG;
#pragma unroll
                        for (int o = 0; o < OG / 2; ++o) {
                            acc2[o] = __builtin_elementwise_fma(f32x2{wc[2 * o], wc[2 * o + 1]}, f32x2{val.x, val.x}, acc2[o]);
                            acc2[o] = __builtin_elementwise_fma(f32x2{wc[OG + 2 * o], wc[OG + 2 * o + 1]}, f32x2{val.y, val.y}, acc2[o]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int o = 0; o < OG / 2; ++o) acc[2 * o] = acc2[o].x, acc[2 * o + 1] = acc2[o].y;
    } else if constexpr (VEC) {
        // fp32 features: the round-2 form (64-bit addresses, library tanhf / expf, weights from LDS).  The half-precision form above
        // measured 7-30 % SLOWER here on the same box (1.47 / 0.63 / 0.19 ms against 1.37 / 0.48 / 0.15 at the three ICIP2024 levels):
        // its shorter instruction stream puts more gathers in flight at once, and this kernel loses L1 hits when it does.
        constexpr int TB = (MAXT > 512 || CG > 8) ? 1 : 3;       // taps per batch (divides 9): 12-24 16-byte gathers in flight per lane
        constexpr int V = CG / 4;                                // gathers per corner: 16 bytes, four channels each
#pragma unroll 1
        for (int k0 = 0; k0 < 9; k0 += TB) {     // (rolled: unrolled, the compiler hoists all 9 * CG * OG weight reads and spills)
            Tap q[TB];
            f32x4 v[TB][4][V];
#pragma unroll
            for (int j = 0; j < TB; ++j) {
                q[j] = tap(k0 + j);
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    v[j][0][c] = *reinterpret_cast<const f32x4 *>(q[j].p1 + 16 * c);
                    v[j][1][c] = *reinterpret_cast<const f32x4 *>(q[j].p2 + 16 * c);
                    v[j][2][c] = *reinterpret_cast<const f32x4 *>(q[j].p3 + 16 * c);
                    v[j][3][c] = *reinterpret_cast<const f32x4 *>(q[j].p4 + 16 * c);
                }
            }
#pragma unroll
            for (int j = 0; j < TB; ++j) {
                const float *wk = wsm + (k0 + j) * CG * OG;
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
                    const f32x4 v1 = q[j].tl ? v[j][0][c] : z, v2 = q[j].tr ? v[j][1][c] : z;
                    const f32x4 v3 = q[j].bl ? v[j][2][c] : z, v4 = q[j].br ? v[j][3][c] : z;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        // (a tap outside the image contributes nothing, whatever its modulation value)
                        const float val = q[j].ok ? (q[j].w1 * v1[e] + q[j].w2 * v2[e] + q[j].w3 * v3[e] + q[j].w4 * v4[e]) * q[j].m : 0.0f;
#pragma unroll
                        for (int o = 0; o < OG; ++o) acc[o] = fmaf(wk[(4 * c + e) * OG + o], val, acc[o]);
                    }
                }
            }
        }
    } else {
#pragma unroll 3
        for (int k = 0; k < 9; ++k) {
            const Tap q = tap(k);
            if (!q.ok) continue;
            const float *wk = wsm + k * CG * OG;
#pragma unroll
            for (int c = 0; c < CG; ++c) {
                const float *f1 = reinterpret_cast<const float *>(q.p1), *f2 = reinterpret_cast<const float *>(q.p2);
                const float *f3 = reinterpret_cast<const float *>(q.p3), *f4 = reinterpret_cast<const float *>(q.p4);
                const float v1 = q.tl ? f1[c] : 0.0f, v2 = q.tr ? f2[c] : 0.0f;
                const float v3 = q.bl ? f3[c] : 0.0f, v4 = q.br ? f4[c] : 0.0f;
                const float val = (q.w1 * v1 + q.w2 * v2 + q.w3 * v3 + q.w4 * v4) * q.m;
#pragma unroll
                for (int o = 0; o < OG; ++o) acc[o] = fmaf(wk[c * OG + o], val, acc[o]);
            }
        }
    }
    float *outp = a.out.p + view_off(a.out, n, y, x) + g * OG;
#pragma unroll
    for (int o = 0; o < OG; ++o) outp[o] = acc[o];
}

// ---- which instance runs --------------------------------------------------------------------------------------------------------
// The whole rule, from seven integers: what vc_deform_select exports, what the launcher follows and -- through reachable() -- the list
// of instances this file compiles.  tests/test_deform_routing_cpu.py pins every row of it (tests/golden/deform_routes.json).
#define VC_DEFORM_SHAPES(X) /* (cg, og): */ X(4, 2) X(4, 4) X(8, 4) /* C = 64 (level 1) */ X(12, 6) /* C = 96 (level 2) */ \
    X(16, 8) /* C = 128 (level 3) */ X(8, 8) X(16, 4) X(12, 12) /* C = 96 (ICIP2023 level 3) */

constexpr int route(bool vec, int rv, int maxt, bool xh) { return (int)vec | rv << 1 | (maxt == 512) << 4 | (int)xh << 5; }

constexpr int select_route(int mode, int cg, int og, int groups, int x_half, bool vec, int rv)
{
#define X(CG, OG) (cg == CG && og == OG) ||
    const bool shape = VC_DEFORM_SHAPES(X) false;
#undef X
    if (mode == MODE_GENERIC) rv = 1;                                          // no records
    if (mode < MODE_GENERIC || mode > MODE_PAIR || x_half < 0 || x_half > 2 || (rv != 1 && rv != 2 && rv != 4)) return VC_EINVAL;
    if (!shape || groups < 2 || groups % 2 || groups > 32) return VC_EINVAL;   // one wave per group of a reference, 1024 threads at most
    const int half = groups / 2;
    while ((27 * half) % rv) rv /= 2;                                          // whole pieces of the 27 * half floats of a record
    // up to 8 groups per reference (the models' shape) a lane may have 256 registers: MAXT = 512
    const bool small = half <= 8;
    // 12 -> 12 channels per group: 144 products per tap and channel next to the gathered values.  The scalar form does not fit the 128
    // registers of a 1024-thread workgroup (384 bytes per lane spilled), so this pair exists with the 512-thread bound only
    const bool big = cg * og > 128;
    if (big && !small) return VC_EINVAL;
    if (x_half) {
        // half features: the fast instance (vector gathers, 16-byte record pieces, 512 threads) or nothing, no slower form behind it.
        // Offset diversity on interleaved or planar ones, every shape but (12, 12); the pair on planar ones at the three shapes of
        // the ICIP2023 model.
        const bool served = mode == MODE_OD ? !big : mode == MODE_PAIR && x_half == 2 && cg == og && (cg == 4 || cg == 8 || cg == 12);
        return served && vec && small && rv == 4 ? route(true, 4, 512, true) : VC_EINVAL;
    }
    // MAXT = 512 leaves the vector form the register file for batched gathers (three taps in flight; cg > 8: one); 1024 keeps 128
    // registers and gathers one tap at a time.  Below (12, 12) the scalar form and 8-byte record pieces (raw tensors 8 bytes off,
    // records of 54 or 270 floats) have the 1024-thread instances only.
    const bool t512 = big || (vec && small && rv != 2);
    return route(vec, rv, t512 ? 512 : 1024, false);
}

// an instance exists iff the rule can name it (at 8 and 16 groups per reference every record width divides the record)
constexpr bool reachable(int mode, int cg, int og, int code)
{
    for (int groups = 16; groups <= 32; groups += 16)
        for (int x_half = 0; x_half < 3; ++x_half)
            for (int vec = 0; vec < 2; ++vec)
                for (int rv = 1; rv <= 4; rv *= 2)
                    if (select_route(mode, cg, og, groups, x_half, vec != 0, rv) == code) return true;
    return false;
}

typedef void (*deform_kernel)(DeformArgs);

// route code -> k_deform<CG, OG, MODE, VEC, RV, MAXT, XH>, the inverse of route()
template <int CG, int OG, int MODE, int CODE = 0> deform_kernel instance(int code)
{
    if constexpr (CODE < 64) {
        if constexpr (reachable(MODE, CG, OG, CODE)) {
            if (code == CODE) return k_deform<CG, OG, MODE, (CODE & 1) != 0, (CODE >> 1) & 7, (CODE & 16) ? 512 : 1024, (CODE & 32) != 0>;
        }
        return instance<CG, OG, MODE, CODE + 1>(code);
    } else {
        return nullptr;
    }
}

// `width` elements of `esz` bytes at a time: the pointer on such a boundary, the strides (in elements) whole multiples
inline bool pieces_ok(const vc_view &v, int width, int esz = 4)
{
    return reinterpret_cast<uintptr_t>(v.p) % (width * esz) == 0 && v.sn % width == 0 && v.sh % width == 0 && v.sw % width == 0;
}

// Largest LDS allocation of a workgroup on the current device in bytes, queried once per device (0: the query failed).
inline size_t lds_limit()
{
    static std::atomic<int> cached[VC_MAX_DEVICES];
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= VC_MAX_DEVICES) {
        (void)hipGetLastError();
        return 0;
    }
    if ((v = cached[dev].load(std::memory_order_relaxed)) > 0) return (size_t)v;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v <= 0) {
        (void)hipGetLastError();
        return 0;
    }
    cached[dev].store(v, std::memory_order_relaxed);
    return (size_t)v;
}

template <int MODE> int launch(hipStream_t st, DeformArgs a, int cg, int og)
{
    const int half = a.groups / 2, esz = a.x_half ? 2 : 4;
    // 16-byte gathers of four floats -- or of eight halves that are only 8-byte aligned, which is legal and all that can be asked: a
    // group's 2 * cg bytes start 8-byte aligned anyway (cg = 4, 12: every other group).  (Every cg served is a multiple of 4.)
    const bool vec = pieces_ok(a.x1, 4, esz) && pieces_ok(a.x2, 4, esz);
    // width of the record pieces: what the alignment of the raw offset tensors allows (the rule lowers it to the record length)
    int rv = 4;
    while (rv > 1 && !(pieces_ok(a.off1, rv) && pieces_ok(a.off2, rv))) rv /= 2;
    const int code = select_route(MODE, cg, og, a.groups, a.x_half, vec, rv);
    if (code < 0) return code;
    const bool xh = (code & 32) != 0;
    // half-precision features: 32-bit byte offsets inside one image of the features (24-bit row / pixel multiplies)
    auto fits32 = [&](const vc_view &v) {
        return (long long)v.h * v.sh * 2 * (a.x_half == 2 ? half : 1) < (1ll << 32) && v.sh * 2 < (1ll << 24) && v.sw * 2 < (1ll << 24) && v.h < (1 << 24) && v.w < (1 << 24);
    };
    if (xh && !(fits32(a.x1) && fits32(a.x2))) return VC_EINVAL;
    // (the half-precision body reads its weights through the scalar cache: the 64 records alone)
    const size_t lds = ((xh ? (size_t)0 : (size_t)half * 9 * cg * og) + (MODE != MODE_GENERIC ? 64 * (27 * half + 1) : 0)) * sizeof(float);
    // more LDS than a workgroup of this device can have (fused, 32 groups of 16 -> 8 channels: 184 KB) is a shape this library does
    // not serve: refused here, before any launch, like every other unsupported shape
    if (lds > 64 * 1024 && lds > lds_limit()) return VC_EINVAL;
    deform_kernel kern = nullptr;
    switch (cg * 16 + og) {
#define X(CG, OG) case CG * 16 + OG: kern = instance<CG, OG, MODE>(code); break;
        VC_DEFORM_SHAPES(X)
#undef X
    }
    if (!kern) return VC_EINVAL;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();                       // (consumed here: the next launch check of the library must not report it as its own)
        return VC_ELAUNCH;
    }
    a.gstride = a.x_half == 2 ? (unsigned)((long long)a.x1.h * a.x1.sh * 2) : (unsigned)(cg * esz);
    // pixels per wave: 4 x 16 on group-planar features, 8 x 8 on pixel-interleaved ones (measured against each other and 2 x 32, 1 x 64)
    a.twl = a.x_half == 2 ? 4 : 3;
    const int tw = 1 << a.twl, th = 64 >> a.twl;
    const unsigned tiles = (unsigned)(((a.out.h + th - 1) / th) * ((a.out.w + tw - 1) / tw));
    hipLaunchKernelGGL(kern, dim3(tiles, 2u, (unsigned)a.out.n), dim3((unsigned)(64 * half)), lds, st, a);
    return hipGetLastError() == hipSuccess ? VC_OK : VC_ELAUNCH;
}

// What the five fused entry points share: the argument contract, checked once, and the kernel's arguments.  MODE_OD with its flow
// fields, MODE_PAIR without (flow1 / flow2 unused); x_half = 2: x1 / x2 describe ONE group's plane of a dense [n][G/2][h][w][cg] tensor.
int fused(int mode, int x_half, vc_stream s, vc_view x1, vc_view raw1, vc_view flow1, vc_view x2, vc_view raw2, vc_view flow2,
          float magnitude, const float *wpk, const float *bias, int groups, vc_view out)
{
    const bool od = mode == MODE_OD;
    if (!x1.p || !x2.p || !raw1.p || !raw2.p || !wpk || !out.p || (od && (!flow1.p || !flow2.p))) return VC_EINVAL;
    if (groups < 2 || groups % 2) return VC_EINVAL;
    const int half = groups / 2;
    if (x_half == 2) {
        for (const vc_view *v : {&x1, &x2})
            if (v->sw != v->c || v->sh != (long long)v->w * v->c || v->sn != (long long)half * v->h * v->sh) return VC_EINVAL;
        if (x1.c != x2.c) return VC_EINVAL;
        x1.c *= half, x2.c *= half;
    }
    if (x1.c != x2.c || x1.c % half || out.c % groups || raw1.c != 27 * half || raw2.c != 27 * half) return VC_EINVAL;
    if (od && (flow1.c < 2 || flow2.c < 2)) return VC_EINVAL;
    auto sized = [&](const vc_view &v) { return v.h == out.h && v.w == out.w && v.n == out.n; };
    if (!sized(x1) || !sized(x2) || !sized(raw1) || !sized(raw2) || (od && !(sized(flow1) && sized(flow2)))) return VC_EINVAL;
    DeformArgs a = {};
    a.x1 = x1;
    a.x2 = x2;
    a.off1 = raw1;
    a.off2 = raw2;
    a.flow1 = flow1;
    a.flow2 = flow2;
    a.out = out;
    a.wpk = wpk;
    a.bias = bias;
    a.magnitude = magnitude;
    a.groups = groups;
    a.x_half = x_half;
    const int cg = x1.c / half, og = out.c / groups;
    return od ? launch<MODE_OD>(as_stream(s), a, cg, og) : launch<MODE_PAIR>(as_stream(s), a, cg, og);
}

}  // namespace

extern "C" int vc_deform_select(int mode, int cg, int og, int groups, int x_half, int vec, int rv)
{
    return select_route(mode, cg, og, groups, x_half, vec != 0, rv);
}

extern "C" int vc_deform_pack_weights(const float *w, int cout, int cg, int groups, float *dst)
{
    if (!w || !dst || groups < 1 || cout % groups || cg < 1) return VC_EINVAL;
    const int og = cout / groups;
    for (int g = 0; g < groups; ++g)
        for (int k = 0; k < 9; ++k)
            for (int c = 0; c < cg; ++c)
                for (int o = 0; o < og; ++o)
                    dst[(((long long)g * 9 + k) * cg + c) * og + o] = w[(((long long)(g * og + o)) * cg + c) * 9 + k];
    return VC_OK;
}

extern "C" int vc_deform_conv2d(vc_stream s, vc_view in, vc_view offset, vc_view mask, const float *wpk, const float *bias,
                                int groups, vc_view out)
{
    if (!in.p || !offset.p || !wpk || !out.p || groups < 2 || groups % 2) return VC_EINVAL;
    if (in.c % groups || out.c % groups || offset.c != groups * 18 || (mask.p && mask.c != groups * 9)) return VC_EINVAL;
    if (in.h != out.h || in.w != out.w || offset.h != out.h || offset.w != out.w || in.n != out.n || offset.n != out.n)
        return VC_EINVAL;
    if (mask.p && (mask.h != out.h || mask.w != out.w || mask.n != out.n)) return VC_EINVAL;
    const int cg = in.c / groups, og = out.c / groups, half = groups / 2;
    DeformArgs a = {};
    a.x1 = in;
    a.x2 = in;
    a.x2.p = in.p + half * cg;
    a.off1 = offset;
    a.off2 = offset;
    a.off2.p = offset.p + half * 18;
    a.msk1 = mask;
    a.msk2 = mask;
    if (mask.p) a.msk2.p = mask.p + half * 9;
    a.out = out;
    a.wpk = wpk;
    a.bias = bias;
    a.groups = groups;
    return launch<MODE_GENERIC>(as_stream(s), a, cg, og);
}

extern "C" int vc_offset_diversity(vc_stream s, vc_view x1, vc_view raw1, vc_view flow1, vc_view x2, vc_view raw2,
                                   vc_view flow2, float magnitude, const float *wpk, const float *bias, int groups,
                                   vc_view out)
{
    return fused(MODE_OD, 0, s, x1, raw1, flow1, x2, raw2, flow2, magnitude, wpk, bias, groups, out);
}

// The same with HALF-precision features: x1.p / x2.p point at _Float16 tensors (strides in elements; vc_to_half makes one).
// fp16 path only -- the gathered values are the features rounded to half, everything else (offsets, modulation, bilinear
// weights, accumulation) stays fp32; offsets / output as in vc_offset_diversity.
extern "C" int vc_offset_diversity_hx(vc_stream s, vc_view x1, vc_view raw1, vc_view flow1, vc_view x2, vc_view raw2,
                                      vc_view flow2, float magnitude, const float *wpk, const float *bias, int groups,
                                      vc_view out)
{
    return fused(MODE_OD, 1, s, x1, raw1, flow1, x2, raw2, flow2, magnitude, wpk, bias, groups, out);
}

// The same on GROUP-PLANAR half features ([n][G/2][h][w][cg], vc_to_half_planar): x1 / x2 describe ONE group's plane (c = cg, sw = cg,
// sh = w * cg, sn = (G/2) * h * w * cg; the planes of an image follow one another).  Neighbouring pixels of a group are then 2 * cg bytes
// apart instead of a whole pixel: the 64 lanes of a gather (a 4 x 16 pixel tile of one group) meet 8-16 cache lines instead of 64.
extern "C" int vc_offset_diversity_hxp(vc_stream s, vc_view x1, vc_view raw1, vc_view flow1, vc_view x2, vc_view raw2,
                                       vc_view flow2, float magnitude, const float *wpk, const float *bias, int groups,
                                       vc_view out)
{
    return fused(MODE_OD, 2, s, x1, raw1, flow1, x2, raw2, flow2, magnitude, wpk, bias, groups, out);
}

// Two plain modulated DeformConv2d(c, c, 3, padding=1, groups=G/2) layers on two inputs with their outputs concatenated (ICIP2023
// DeformB.get_deformed_maps, m.py:72-86) as ONE grouped deformable convolution with G groups: groups [0, G/2) read x1 with the first
// layer's weights, groups [G/2, G) read x2 with the second layer's.  raw_r = that reference's half of the offset head, the record
// [x-block | y-block | mask-block] of 9 * G/2 channels each: cat(x-block, y-block) IS torchvision's offset tensor, the mask block goes
// through the logistic; no tanh, no magnitude, no flow.  fp32 features.
extern "C" int vc_deform_pair(vc_stream s, vc_view x1, vc_view raw1, vc_view x2, vc_view raw2, const float *wpk, const float *bias,
                              int groups, vc_view out)
{
    return fused(MODE_PAIR, 0, s, x1, raw1, vc_view{}, x2, raw2, vc_view{}, 0.0f, wpk, bias, groups, out);
}

// The same on GROUP-PLANAR half features (fp16 path; the view contract of vc_offset_diversity_hxp).  One instance per shape of the
// ICIP2023 model -- k_deform<cg, cg, MODE_PAIR, true, 4, 512, true> for cg = 4, 8, 12 -- and no slower form behind it: whatever that
// instance does not serve is refused by select_route, before any launch.
extern "C" int vc_deform_pair_hxp(vc_stream s, vc_view x1, vc_view raw1, vc_view x2, vc_view raw2, const float *wpk, const float *bias,
                                  int groups, vc_view out)
{
    return fused(MODE_PAIR, 2, s, x1, raw1, vc_view{}, x2, raw2, vc_view{}, 0.0f, wpk, bias, groups, out);
}


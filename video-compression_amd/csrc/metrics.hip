// Quality metrics of the evaluation loops that are more than a sum of squared errors (gfx950).
//
// MS-SSIM -- the public pytorch-msssim `ms_ssim` with its default arguments, on the images the PSNR kernel sees
// (vc_psnr_uint8, entropy.hip), per image:
//   1. the [:h,:w] crop of two CHW fp32 images (row pitch W, plane pitch H*W); quantize=1: every value becomes
//      rint(clamp(v,0,1)*255) (half to even); quantize=0: v*255 without a clamp.
//   2. L = 255, C1 = (0.01 L)^2, C2 = (0.03 L)^2; window g[i] = exp(-(i-5)^2 / (2 * 1.5^2)), 11 taps, normalised to sum 1,
//      applied separably as a "valid" filter F per channel: the map of a p x q plane is (p-10) x (q-10).
//   3. per scale and channel: mu1 = F(X), mu2 = F(Y), s1 = F(XX) - mu1^2, s2 = F(YY) - mu2^2, s12 = F(XY) - mu1 mu2,
//      cs = (2 s12 + C2) / (s1 + s2 + C2), ssim = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * cs; the scale's term is the mean
//      of the cs map (scales 0..3) or of the ssim map (scale 4), passed through max(., 0).
//   4. between scales both images go through a 2x2 / stride-2 average pool that pads ONE zero row on top when the height is
//      odd and one zero column on the left when the width is odd (the zeros count: the divisor is always 4); p -> p/2 + (p&1).
//   5. per channel prod_k term_k ^ w_k, w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) (a zero term gives 0); the image's
//      value is the mean over channels.  min(h,w) > 160 is required (the last map must not be empty).
//
// Layout: ONE launch per scale + one single-workgroup finishing launch, for any number of images.  A workgroup of a scale
// launch owns a 32 x 16 tile of the map of one plane: it stages the 42 x 26 input pixels of both images in LDS (quantised on
// load at scale 0), writes the pooled pixels of the NEXT scale whose 2x2 cell starts inside its 32 x 16 input tile (the last
// tile of a row / column also takes the 10-pixel rest; cell -1 goes to tile 0), runs the window over the rows (five sums in
// fp64, kept in LDS) and then over the columns, forms cs (ssim at the last scale), reduces over the workgroup in double and
// writes one partial to its own slot.  The finishing launch sums the slots in a fixed order: no floating-point atomics, same
// bits on every call.  The five window sums are fp64 because F(XX) - mu^2 cancels on flat content (fp32: 7e-4 off there).
#include "common.h"
#include <math.h>

namespace {

constexpr int MS_TW = 32, MS_TH = 16;             // map tile of a workgroup (both even: pooled cells never straddle tile origins)
constexpr int MS_IW = MS_TW + 10, MS_IH = MS_TH + 10;
constexpr int MS_PITCH = MS_IW + 1;               // 43 floats: the 4-pixel-strided reads of the row pass fall on distinct banks
constexpr int MS_BLOCK = 256;
constexpr int MS_SCALES = 5;

struct MsScaleArgs {
    const float *a, *b;                 // inputs: the frames (scale 0) or the pooled planes of this scale
    long long image_pitch, plane_pitch; // in floats
    int row_pitch, p, q;                // plane size p x q
    int mode;                           // 0: values as stored (pooled planes), 1: v * 255, 2: rint(clamp(v,0,1) * 255)
    float *pa, *pb;                     // pooled planes of the next scale, dense [n][C][ps][qs]; null at the last scale
    int ps, qs;
    double *partial;                    // [n][C][tiles]
    int tiles_x, tiles_y;
    int last;                           // the last scale: the ssim map instead of the cs map
    double g[11];
};

__device__ __forceinline__ float ms_fetch(const float *__restrict__ src, long long off, int mode)
{
    const float v = src[off];
    if (mode == 0) return v;
    if (mode == 1) return v * 255.0f;
    return rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f);
}

__global__ void __launch_bounds__(MS_BLOCK) k_msssim_scale(const MsScaleArgs A)
{
    __shared__ float sa[MS_IH * MS_PITCH], sb[MS_IH * MS_PITCH];
    __shared__ double sh[5][MS_IH][MS_TW];
    __shared__ double red[MS_BLOCK / 64];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % A.tiles_x, ty = blockIdx.x / A.tiles_x;
    const int x0 = tx * MS_TW, y0 = ty * MS_TH;
    const int plane = blockIdx.z * gridDim.y + blockIdx.y;
    const long long base = (long long)blockIdx.z * A.image_pitch + (long long)blockIdx.y * A.plane_pitch;

    // ---- the tile and its apron of both images (zero outside the plane: those taps only reach map pixels that are masked out)
    for (int i = tid; i < MS_IH * MS_IW; i += MS_BLOCK) {
        const int r = i / MS_IW, c = i - r * MS_IW;
        const int y = y0 + r, x = x0 + c;
        float va = 0.0f, vb = 0.0f;
        if (y < A.p && x < A.q) {
            const long long o = base + (long long)y * A.row_pitch + x;
            va = ms_fetch(A.a, o, A.mode);
            vb = ms_fetch(A.b, o, A.mode);
        }
        sa[r * MS_PITCH + c] = va;
        sb[r * MS_PITCH + c] = vb;
    }
    __syncthreads();

    // ---- this tile's share of the next scale: the 2x2 cells whose first row / column lies in the 32 x 16 input tile
    if (A.pa) {
        const int py = A.p & 1, px = A.q & 1;
        const int i0 = ty == 0 ? 0 : (y0 + py + 1) / 2, i1 = ty == A.tiles_y - 1 ? A.ps : (y0 + MS_TH + py + 1) / 2;
        const int j0 = tx == 0 ? 0 : (x0 + px + 1) / 2, j1 = tx == A.tiles_x - 1 ? A.qs : (x0 + MS_TW + px + 1) / 2;
        const int nj = j1 - j0, cells = (i1 - i0) * nj;
        float *__restrict__ da = A.pa + (long long)plane * A.ps * A.qs;
        float *__restrict__ db = A.pb + (long long)plane * A.ps * A.qs;
        for (int k = tid; k < cells; k += MS_BLOCK) {
            const int i = i0 + k / nj, j = j0 + k % nj;
            const int r = 2 * i - py - y0, c = 2 * j - px - x0;        // -1 only for the padded zero row / column of tile 0
            float ua = 0.0f, ub = 0.0f;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx)
                    if (r + dy >= 0 && c + dx >= 0) {
                        ua += sa[(r + dy) * MS_PITCH + c + dx];
                        ub += sb[(r + dy) * MS_PITCH + c + dx];
                    }
            da[(long long)i * A.qs + j] = 0.25f * ua;
            db[(long long)i * A.qs + j] = 0.25f * ub;
        }
    }

    // ---- window along the rows: a thread forms four neighbouring outputs of one row from 14 pixels of each image
    if (tid < MS_IH * (MS_TW / 4)) {
        const int r = tid / (MS_TW / 4), c = 4 * (tid % (MS_TW / 4));
        double acc[5][4];
#pragma unroll
        for (int k = 0; k < 5; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[k][e] = 0.0;
#pragma unroll
        for (int t = 0; t < 14; ++t) {
            const double x = (double)sa[r * MS_PITCH + c + t], y = (double)sb[r * MS_PITCH + c + t];
            const double xx = x * x, yy = y * y, xy = x * y;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int tap = t - e;
                if (tap >= 0 && tap < 11) {
                    const double g = A.g[tap];
                    acc[0][e] = fma(g, x, acc[0][e]);
                    acc[1][e] = fma(g, y, acc[1][e]);
                    acc[2][e] = fma(g, xx, acc[2][e]);
                    acc[3][e] = fma(g, yy, acc[3][e]);
                    acc[4][e] = fma(g, xy, acc[4][e]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 5; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) sh[k][r][c + e] = acc[k][e];
    }
    __syncthreads();

    // ---- window along the columns: a thread forms two map pixels, one below the other, from 12 rows
    const int x = tid & (MS_TW - 1), y = 2 * (tid / MS_TW);
    double f[5][2];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        double v0 = 0.0, v1 = 0.0;
#pragma unroll
        for (int t = 0; t < 12; ++t) {
            const double v = sh[k][y + t][x];
            if (t < 11) v0 = fma(A.g[t], v, v0);
            if (t > 0) v1 = fma(A.g[t - 1], v, v1);
        }
        f[k][0] = v0;
        f[k][1] = v1;
    }
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    double sum = 0.0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const double mu1 = f[0][e], mu2 = f[1][e];
        const double m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
        const double s1 = f[2][e] - m11, s2 = f[3][e] - m22, s12 = f[4][e] - m12;
        double v = (2.0 * s12 + C2) / (s1 + s2 + C2);
        if (A.last) v *= (2.0 * m12 + C1) / (m11 + m22 + C1);
        if (y0 + y + e < A.p - 10 && x0 + x < A.q - 10) sum += v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        double r = 0.0;
        for (int w = 0; w < MS_BLOCK / 64; ++w) r += red[w];
        A.partial[(long long)plane * (A.tiles_x * A.tiles_y) + blockIdx.x] = r;
    }
}

struct MsFinishArgs {
    const double *partial[MS_SCALES];   // per scale [n][C][tiles]
    int tiles[MS_SCALES];
    double inv_count[MS_SCALES];        // 1 / pixels of the scale's map
    int n, C;
    double *terms;                      // [n][5][C] (workspace)
    double *terms_out;                  // nullable copy for the caller
    double *out;                        // [n]
};

__global__ void __launch_bounds__(MS_BLOCK) k_msssim_finish(const MsFinishArgs A)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int total = A.n * A.C * MS_SCALES;
    // one wave per (image, scale, channel): lane l adds slots l, l + 64, ... in order, then the fixed shuffle tree
    for (int idx = wave; idx < total; idx += MS_BLOCK / 64) {
        const int c = idx % A.C, s = (idx / A.C) % MS_SCALES, img = idx / (A.C * MS_SCALES);
        const double *__restrict__ src = A.partial[s] + ((long long)img * A.C + c) * A.tiles[s];
        double v = 0.0;
        for (int j = lane; j < A.tiles[s]; j += 64) v += src[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) {
            const double term = fmax(v * A.inv_count[s], 0.0);
            A.terms[idx] = term;
            if (A.terms_out) A.terms_out[idx] = term;
        }
    }
    __threadfence_block();
    __syncthreads();
    const double wgt[MS_SCALES] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    for (int img = threadIdx.x; img < A.n; img += MS_BLOCK) {
        double acc = 0.0;
        for (int c = 0; c < A.C; ++c) {
            double prod = 1.0;
            for (int s = 0; s < MS_SCALES; ++s) {
                const double t = A.terms[((long long)img * MS_SCALES + s) * A.C + c];
                prod *= t > 0.0 ? pow(t, wgt[s]) : 0.0;
            }
            acc += prod;
        }
        A.out[img] = acc / (double)A.C;
    }
}

struct MsPlan {
    int p[MS_SCALES], q[MS_SCALES], tiles_x[MS_SCALES], tiles_y[MS_SCALES];
    size_t partial_off[MS_SCALES], terms_off, plane_off[MS_SCALES][2];   // bytes; plane_off[0] unused
    size_t bytes;
};

bool ms_plan(int n, int channels, int h, int w, MsPlan &P)
{
    if (n < 1 || channels < 1 || h <= 160 || w <= 160) return false;
    const size_t planes = (size_t)n * channels;
    size_t off = 0;
    for (int s = 0; s < MS_SCALES; ++s) {
        P.p[s] = s ? P.p[s - 1] / 2 + (P.p[s - 1] & 1) : h;
        P.q[s] = s ? P.q[s - 1] / 2 + (P.q[s - 1] & 1) : w;
        P.tiles_x[s] = (P.q[s] - 10 + MS_TW - 1) / MS_TW;
        P.tiles_y[s] = (P.p[s] - 10 + MS_TH - 1) / MS_TH;
        P.partial_off[s] = off;
        off += planes * P.tiles_x[s] * P.tiles_y[s] * sizeof(double);
    }
    P.terms_off = off;
    off += planes * MS_SCALES * sizeof(double);
    for (int s = 1; s < MS_SCALES; ++s)
        for (int i = 0; i < 2; ++i) {
            P.plane_off[s][i] = off;
            off += (planes * P.p[s] * P.q[s] * sizeof(float) + 15) / 16 * 16;
        }
    P.bytes = off;
    return true;
}

}  // namespace

extern "C" size_t vc_msssim_workspace_bytes(int n, int channels, int h, int w)
{
    MsPlan P;
    return ms_plan(n, channels, h, w, P) ? P.bytes : 0;
}

extern "C" int vc_msssim(vc_stream s, const float *a, const float *b, int n, int channels, int H, int W, int h, int w,
                         long long image_pitch, int quantize, void *workspace, size_t workspace_bytes, double *terms_out,
                         double *msssim_out)
{
    if (!a || !b || !workspace || !msssim_out) return VC_EINVAL;
    if (n < 1 || n > 65535 || channels < 1 || channels > 65535 || h > H || w > W || (quantize != 0 && quantize != 1)) return VC_EINVAL;
    if (image_pitch < (long long)channels * H * W) return VC_EINVAL;
    MsPlan P;
    if (!ms_plan(n, channels, h, w, P) || workspace_bytes < P.bytes) return VC_EINVAL;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    double g[11], gs = 0.0;
    for (int i = 0; i < 11; ++i) gs += g[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
    MsFinishArgs F = {};
    for (int k = 0; k < MS_SCALES; ++k) {
        MsScaleArgs A = {};
        if (k == 0) {
            A.a = a, A.b = b;
            A.image_pitch = image_pitch, A.plane_pitch = (long long)H * W, A.row_pitch = W;
            A.mode = quantize ? 2 : 1;
        } else {
            A.a = reinterpret_cast<const float *>(ws + P.plane_off[k][0]);
            A.b = reinterpret_cast<const float *>(ws + P.plane_off[k][1]);
            A.plane_pitch = (long long)P.p[k] * P.q[k], A.image_pitch = A.plane_pitch * channels, A.row_pitch = P.q[k];
            A.mode = 0;
        }
        A.p = P.p[k], A.q = P.q[k];
        if (k + 1 < MS_SCALES) {
            A.pa = reinterpret_cast<float *>(ws + P.plane_off[k + 1][0]);
            A.pb = reinterpret_cast<float *>(ws + P.plane_off[k + 1][1]);
            A.ps = P.p[k + 1], A.qs = P.q[k + 1];
        }
        A.partial = reinterpret_cast<double *>(ws + P.partial_off[k]);
        A.tiles_x = P.tiles_x[k], A.tiles_y = P.tiles_y[k];
        A.last = k == MS_SCALES - 1;
        for (int i = 0; i < 11; ++i) A.g[i] = g[i] / gs;
        hipLaunchKernelGGL(k_msssim_scale, dim3(A.tiles_x * A.tiles_y, channels, n), dim3(MS_BLOCK), 0, as_stream(s), A);
        VC_LAUNCH_CHECK();
        F.partial[k] = A.partial;
        F.tiles[k] = A.tiles_x * A.tiles_y;
        F.inv_count[k] = 1.0 / ((double)(A.p - 10) * (double)(A.q - 10));
    }
    F.n = n, F.C = channels;
    F.terms = reinterpret_cast<double *>(ws + P.terms_off);
    F.terms_out = terms_out;
    F.out = msssim_out;
    hipLaunchKernelGGL(k_msssim_finish, dim3(1), dim3(MS_BLOCK), 0, as_stream(s), F);
    VC_LAUNCH_CHECK();
    return VC_OK;
}

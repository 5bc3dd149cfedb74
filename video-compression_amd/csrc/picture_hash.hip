// Decoded picture hash (vc_picture_hash / vc_picture_hash_host; include/vc_hip.h, "Decoded picture hash").
//
//   mix(t):  t += 0x9E3779B97F4A7C15;  t = (t ^ (t >> 30)) * 0xBF58476D1CE4E5B9;  t = (t ^ (t >> 27)) * 0x94D049BB133111EB;
//            return t ^ (t >> 31)                                                          (uint64, wrapping)
//   hash(w[0..count)) = mix(count) + sum_i mix((uint64(i) << 32) | w[i])                   (mod 2^64)
//
// A sum of per-word terms modulo 2^64: every summation order gives the same bits, so the kernel is free to deal the words to lanes
// as the addresses suit it.  Per image: the words in front of the first 16-byte boundary (0..3 of them) and behind the last whole
// 16-byte group (0..3) are read one by one by the first lanes of the image's first workgroup, everything between as one 16-byte
// load per lane and step.  The word index is the index within the image, whatever the image's phase.  Per-workgroup partial sums
// (plain vector stores), then one finishing workgroup per image that folds the `used` partials in a fixed order and adds
// mix(count): two launches for any n, no atomics, nothing read back.
//
// Cost per word: two 64-bit multiplies by constants (each one 32x32->64 multiply-add and two 32-bit multiplies) and a dozen
// shifts / xors / adds against 4 bytes loaded -- see DESIGN.md section 4h for the measured rate beside a plain copy.
#include "common.h"

#define PH_BLOCK 256
#define PH_SLOTS 1024          // = vc_bits_slots(): the partials of one image

static __host__ __device__ __forceinline__ uint64_t ph_mix(uint64_t t)
{
    t += 0x9E3779B97F4A7C15ull;
    t = (t ^ (t >> 30)) * 0xBF58476D1CE4E5B9ull;
    t = (t ^ (t >> 27)) * 0x94D049BB133111EBull;
    return t ^ (t >> 31);
}

static __host__ __device__ __forceinline__ uint64_t ph_term(uint32_t i, uint32_t w) { return ph_mix(((uint64_t)i << 32) | w); }

extern "C" uint64_t vc_picture_hash_host(const uint32_t *words, size_t count)
{
    if (!words) return 0;
    uint64_t h = ph_mix((uint64_t)count);
    for (size_t i = 0; i < count; ++i) h += ph_term((uint32_t)i, words[i]);
    return h;
}

__device__ __forceinline__ uint64_t ph_block_sum(uint64_t v, uint64_t *sm)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_down((unsigned long long)v, o, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t r = 0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < PH_BLOCK / 64; ++w) r += sm[w];
    }
    return r;          // valid in thread 0
}

// grid (used, n): workgroup (b, img) sums its share of image img into partials[img * PH_SLOTS + b]
__global__ void __launch_bounds__(PH_BLOCK) k_picture_hash(const uint32_t *__restrict__ words, uint32_t count, size_t image_pitch,
                                                           uint64_t *__restrict__ partials)
{
    __shared__ uint64_t sm[PH_BLOCK / 64];
    const uint32_t *p = words + (size_t)blockIdx.y * image_pitch;
    // words in front of the first 16-byte boundary; the pointer is 4-byte aligned
    uint32_t head = (uint32_t)((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u) >> 2;
    if (head > count) head = count;
    const uint32_t nvec = (count - head) >> 2;                 // whole 16-byte groups
    const uint32_t tail0 = head + 4u * nvec;                   // first word behind them; count - tail0 <= 3
    uint64_t acc = 0;
    if (blockIdx.x == 0) {
        const uint32_t t = threadIdx.x;
        if (t < head) acc += ph_term(t, p[t]);
        else if (t >= 4 && t - 4 < count - tail0) acc += ph_term(tail0 + (t - 4), p[tail0 + (t - 4)]);
    }
    const uint4 *pv = reinterpret_cast<const uint4 *>(p + head);
    for (uint32_t v = blockIdx.x * PH_BLOCK + threadIdx.x; v < nvec; v += gridDim.x * PH_BLOCK) {
        const uint4 q = pv[v];
        const uint32_t i = head + 4u * v;
        acc += ph_term(i, q.x) + ph_term(i + 1, q.y) + ph_term(i + 2, q.z) + ph_term(i + 3, q.w);
    }
    const uint64_t r = ph_block_sum(acc, sm);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * PH_SLOTS + blockIdx.x] = r;
}

// grid n: hash_out[img] = mix(count) + the image's `used` partials
__global__ void __launch_bounds__(PH_BLOCK) k_picture_hash_finish(const uint64_t *__restrict__ partials, int used, uint32_t count,
                                                                  uint64_t *__restrict__ hash_out)
{
    __shared__ uint64_t sm[PH_BLOCK / 64];
    uint64_t v = 0;
    for (int j = threadIdx.x; j < used; j += PH_BLOCK) v += partials[(size_t)blockIdx.x * PH_SLOTS + j];
    const uint64_t r = ph_block_sum(v, sm);
    if (threadIdx.x == 0) hash_out[blockIdx.x] = r + ph_mix((uint64_t)count);
}

extern "C" int vc_picture_hash(vc_stream s, const uint32_t *words, int n, size_t count, size_t image_pitch, uint64_t *partials,
                               int slots, uint64_t *hash_out)
{
    if (!words || !partials || !hash_out || n < 1 || n > 65535 || count < 1 || count >= ((size_t)1 << 32) || image_pitch < count) return VC_EINVAL;
    if (slots != PH_SLOTS || slots != vc_bits_slots() || ((uintptr_t)words & 3u)) return VC_EINVAL;
    // one 16-byte load per lane and step; a workgroup for every 4 steps' worth of the image, at most PH_SLOTS
    const size_t groups = (count / 4 + (size_t)PH_BLOCK * 4 - 1) / ((size_t)PH_BLOCK * 4);
    const int used = (int)(groups < 1 ? 1 : groups > PH_SLOTS ? PH_SLOTS : groups);
    hipLaunchKernelGGL(k_picture_hash, dim3(used, n), dim3(PH_BLOCK), 0, as_stream(s), words, (uint32_t)count, image_pitch, partials);
    VC_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_picture_hash_finish, dim3(n), dim3(PH_BLOCK), 0, as_stream(s), partials, used, (uint32_t)count, hash_out);
    VC_LAUNCH_CHECK();
    return VC_OK;
}

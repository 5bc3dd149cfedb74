// Expressions that entropy.hip (vc_gc_indexes, vc_eb_dequant, vc_gc_dequant, ...) and the fused decode kernels of
// rans_device.hip (vc_irans_decode_eb / vc_irans_decode_gc / vc_irans_decode_gc_ckbd) must agree on bit for bit: the scale-table
// index of a scale, the de-quantisation of a decoded integer and the column of a checkerboard position.  One statement of each, included by both translation units.
#pragma once
#include <stdint.h>

// lower_bound_scale of the Gaussian conditional: applied before the index is taken
__device__ __forceinline__ float vc_lower_bound_scale(float s) { return fmaxf(s, 0.11f); }

__device__ __forceinline__ int scale_index(float s, const float *__restrict__ table, int n_scales)
{
    // build_indexes: (n_scales-1) - #{t in table[:-1] : s <= t}; table is ascending, so count from the top
    int idx = n_scales - 1;
    for (int k = 0; k < n_scales - 1; ++k) idx -= (s <= table[k]) ? 1 : 0;
    return idx;
}

// full-resolution column of half-column xs in row y of one checkerboard parity (1 = the anchors, (row + col) odd)
__device__ __forceinline__ int ckbd_column(int xs, int y, int parity) { return 2 * xs + ((y ^ parity) & 1); }

// factorised prior: symbol + the channel's median, then the channel's output gain when one is set
__device__ __forceinline__ float vc_eb_dequant_value(int32_t symbol, float med, const float *__restrict__ out_gain, int c)
{
    const float v = (float)symbol + med;
    return out_gain ? v * out_gain[c] : v;
}

// Gaussian conditional: symbol + mean, then the channel's output gain when one is set
__device__ __forceinline__ float vc_gc_dequant_value(int32_t symbol, float mean, const float *__restrict__ out_gain, int c)
{
    const float v = (float)symbol + mean;
    return out_gain ? v * out_gain[c] : v;
}

// vfa_rotation.h -- the rotation rule of the BEV decode as one device function, shared by vfa_decode.hip (logits read from the dense
// head) and vfa_cellconv.hip (logits computed at the cells): rotation = (float)argmax * (float)(pi / 180), the arg-max over
// s(x) = 1.0f / (1.0f + expf(-x)), the FIRST index that attains the maximum (saturated logits tie at 1.0f), a NaN never wins and
// all NaN gives index 0.
#ifndef VFA_ROTATION_H
#define VFA_ROTATION_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vfa_rotation {

__device__ __forceinline__ float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// The 64 lanes of one wave reduce the n logits o[c * stride], c = 0 .. n - 1, by (sigmoid value, lowest index); every lane returns
// the rotation.
__device__ __forceinline__ float wave_rotation(const float *o, long long stride, int n, int lane)
{
    float best = -1.0f; // below every sigmoid; a NaN never passes `>`
    int best_at = INT32_MAX;
    for (int c = lane; c < n; c += 64) { // (ascending c: the first of equal values stays)
        const float v = sigmoid(o[c * stride]);
        if (v > best) { best = v; best_at = c; }
    }
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) {
        const float v = __shfl_xor(best, step, 64);
        const int at = __shfl_xor(best_at, step, 64);
        if (v > best || (v == best && at < best_at)) { best = v; best_at = at; }
    }
    return (float)(best_at == INT32_MAX ? 0 : best_at) * 0.017453292519943295f; // torch.deg2rad
}

} // namespace vfa_rotation
#endif // VFA_ROTATION_H

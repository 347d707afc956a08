// The zero-padded trilinear tap of hos_trilinear.h WITH its gradient, from the same eight loads: the tracked mesh's Newton solve
// (hos_track.hip).  A header of its own: `trilinear_zero` and the kernels that call it stay as they are, instruction for instruction.
#pragma once
#include <hip/hip_runtime.h>

// Value: the arithmetic of trilinear_zero (same coordinates, tap order, weights and sums).  Gradient (*dx, *dy, *dz): that of the
// trilinear interpolant inside the cell of floor (one-sided on a cell face), in INDEX coordinates (per voxel); the caller scales it
// to its own units.  Per tap v: d/dix = (dx ? +1 : -1) * (wy * wz) * v, and so on; a tap outside the volume is zero in both.
__device__ __forceinline__ float trilinear_zero_grad(const float* __restrict__ vol, int V, float gx, float gy, float gz, float* __restrict__ dx_,
                                                     float* __restrict__ dy_, float* __restrict__ dz_) {
    const float ix = ((gx + 1.f) / 2.f) * (float)(V - 1);
    const float iy = ((gy + 1.f) / 2.f) * (float)(V - 1);
    const float iz = ((gz + 1.f) / 2.f) * (float)(V - 1);
    const float fx = floorf(ix), fy = floorf(iy), fz = floorf(iz);
    *dx_ = 0.f; *dy_ = 0.f; *dz_ = 0.f;
    // NaN / huge coordinates: every tap out of range -> 0
    if (!(fx >= -1.f && fx <= (float)V && fy >= -1.f && fy <= (float)V && fz >= -1.f && fz <= (float)V)) return 0.f;
    const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
    const float wx1 = ix - fx, wy1 = iy - fy, wz1 = iz - fz;
    const float wx0 = (fx + 1.f) - ix, wy0 = (fy + 1.f) - iy, wz0 = (fz + 1.f) - iz;
    float out = 0.f, ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int x = x0 + dx, y = y0 + dy, z = z0 + dz;
                if (x >= 0 && x < V && y >= 0 && y < V && z >= 0 && z < V) {
                    const float wx = dx ? wx1 : wx0, wy = dy ? wy1 : wy0, wz = dz ? wz1 : wz0;
                    const float v = vol[((size_t)z * V + y) * V + x];
                    out += v * (wx * wy * wz);
                    const float tx = v * (wy * wz), ty = v * (wx * wz), tz = v * (wx * wy);
                    ax = dx ? ax + tx : ax - tx;
                    ay = dy ? ay + ty : ay - ty;
                    az = dz ? az + tz : az - tz;
                }
            }
    *dx_ = ax; *dy_ = ay; *dz_ = az;
    return out;
}

// The zero-padded trilinear tap of the motion-weight volume: ONE definition for the backward warp (hos_human.hip) and the canonical
// field of the mesh (hos_mesh.hip), so that the two masks are the same arithmetic bit for bit.
#pragma once
#include <hip/hip_runtime.h>

// F.grid_sample(..., mode='bilinear', padding_mode='zeros', align_corners=True) on one channel of a
// [V,V,V] (z,y,x) volume at normalised (gx,gy,gz); tap order and weights as PyTorch's 3-D kernel.
__device__ __forceinline__ float trilinear_zero(const float* __restrict__ vol, int V, float gx, float gy, float gz) {
    const float ix = ((gx + 1.f) / 2.f) * (float)(V - 1);
    const float iy = ((gy + 1.f) / 2.f) * (float)(V - 1);
    const float iz = ((gz + 1.f) / 2.f) * (float)(V - 1);
    const float fx = floorf(ix), fy = floorf(iy), fz = floorf(iz);
    // NaN / huge coordinates: every tap out of range -> 0
    if (!(fx >= -1.f && fx <= (float)V && fy >= -1.f && fy <= (float)V && fz >= -1.f && fz <= (float)V)) return 0.f;
    const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
    const float wx1 = ix - fx, wy1 = iy - fy, wz1 = iz - fz;
    const float wx0 = (fx + 1.f) - ix, wy0 = (fy + 1.f) - iy, wz0 = (fz + 1.f) - iz;
    float out = 0.f;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int x = x0 + dx, y = y0 + dy, z = z0 + dz;
                if (x >= 0 && x < V && y >= 0 && y < V && z >= 0 && z < V) {
                    const float w = (dx ? wx1 : wx0) * (dy ? wy1 : wy0) * (dz ? wz1 : wz0);
                    out += vol[((size_t)z * V + y) * V + x] * w;
                }
            }
    return out;
}

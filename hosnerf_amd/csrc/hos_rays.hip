// Per-frame ray set-up on the device.  The reference recomputes full-image rays in numpy twice per
// training item plus a six-plane AABB test inside a DataLoader worker and ships them pinned
// (S3/core/data/human_nerf/train.py:513-548, core/utils/camera_util.py:154-265 = `C:`); at the renderer's speed that
// becomes the bottleneck.  Here one thread per pixel:
//   hos_camera_rays  C:154-216  origin -R^T T, direction ((K^-1 [i,j,1]) - T) R - o, unit view direction, and the
//                               mip-NeRF pixel radius  |d(row) - d(row+1)| * 2/sqrt(12)  (last row repeats row H-2)
//   hos_rays_aabb    C:219-265  six-plane AABB (bounds grown by 0.01), a ray is valid iff exactly two of the six
//                               plane hits lie inside the box (+-1e-6); near/far = distances of the two hits / |d|
//   hos_frame_rays_compact   both of the above for one camera and one box, keeping only the rays that hit the box, in pixel
//                               order (the order of ray_mask.nonzero()): per-block counts, a scan of the block counts, a write pass
//   hos_frame_paint             rendered[ray_mask] = rgb over the background colour + to_8b_image, one thread per pixel
// The per-pixel arithmetic lives in the __device__ functions below; every kernel of this file calls the same ones.
// HBM-bound on the outputs: 40 B per pixel (o, d, viewdir, radius) + 12 B (near, far, mask).
#include "hos_common.h"

namespace {

struct Cam { float Kinv[9]; float R[9]; float T[3]; };

__device__ __forceinline__ void pixel_dir(const Cam& c, float i, float j, const float (&o)[3], float (&d)[3]) {
    float pc[3], q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) pc[a] = (i * c.Kinv[a * 3 + 0] + j * c.Kinv[a * 3 + 1]) + c.Kinv[a * 3 + 2];   // xy1 . Kinv^T
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = pc[a] - c.T[a];
#pragma unroll
    for (int b = 0; b < 3; ++b) d[b] = ((q[0] * c.R[0 * 3 + b] + q[1] * c.R[1 * 3 + b]) + q[2] * c.R[2 * 3 + b]) - o[b];   // (pc - T) R - o
}

__device__ __forceinline__ void camera_origin(const Cam& c, float (&o)[3]) {
#pragma unroll
    for (int b = 0; b < 3; ++b) o[b] = -((c.R[0 * 3 + b] * c.T[0] + c.R[1 * 3 + b] * c.T[1]) + c.R[2 * 3 + b] * c.T[2]);     // -R^T T
}

struct Box { float lo[3], hi[3]; };

__host__ __device__ __forceinline__ Box grown_box(float bx0, float by0, float bz0, float bx1, float by1, float bz1) {
    return Box{{bx0 - 0.01f, by0 - 0.01f, bz0 - 0.01f}, {bx1 + 0.01f, by1 + 0.01f, bz1 + 0.01f}};
}

// C:238 clamp of tiny direction components (in `d`; bit a of the return value is set where component a was clamped)
__device__ __forceinline__ int clamp_dir(float (&d)[3]) {
    int clamped = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (fabsf(d[a]) < 1e-5f) { d[a] = 1e-5f; clamped |= 1 << a; }
    return clamped;
}

// C:239-263 for one ray whose direction has been clamped: valid iff exactly two plane hits lie inside the box
__device__ __forceinline__ bool ray_box(const Box& bx, const float (&o)[3], const float (&d)[3], float& near, float& far) {
    const float eps = 1e-6f;
    const float (&lo)[3] = bx.lo;
    const float (&hi)[3] = bx.hi;
    int hits = 0;
    float t[2] = {0.f, 0.f};
#pragma unroll
    for (int side = 0; side < 2; ++side)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float s = ((side ? hi[a] : lo[a]) - o[a]) / d[a];
            const float x = s * d[0] + o[0], y = s * d[1] + o[1], z = s * d[2] + o[2];
            const bool in = x >= lo[0] - eps && x <= hi[0] + eps && y >= lo[1] - eps && y <= hi[1] + eps &&
                            z >= lo[2] - eps && z <= hi[2] + eps;
            if (in) {
                if (hits < 2) {
                    // |p - o| / |d| = |s| (the reference measures both norms explicitly, C:259-262)
                    const float px = x - o[0], py = y - o[1], pz = z - o[2];
                    t[hits] = sqrtf((px * px + py * py) + pz * pz) / sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
                }
                ++hits;
            }
        }
    const bool ok = hits == 2;
    near = ok ? fminf(t[0], t[1]) : 0.f;
    far = ok ? fmaxf(t[0], t[1]) : 0.f;
    return ok;
}

__global__ __launch_bounds__(256) void camera_rays_kernel(Cam c, int H, int W, float* __restrict__ rays_o, float* __restrict__ rays_d,
                                                          float* __restrict__ viewdirs, float* __restrict__ radii) {
    const long n = (long)H * W;
    float o[3];
    camera_origin(c, o);
    float e[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) e[b] = (c.Kinv[0 * 3 + 1] * c.R[0 * 3 + b] + c.Kinv[1 * 3 + 1] * c.R[1 * 3 + b]) + c.Kinv[2 * 3 + 1] * c.R[2 * 3 + b];
    const float radius = sqrtf((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) * 2.f / sqrtf(12.f);
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long)gridDim.x * blockDim.x) {
        const int row = (int)(p / W), col = (int)(p % W);
        float d[3];
        pixel_dir(c, (float)col, (float)row, o, d);
#pragma unroll
        for (int b = 0; b < 3; ++b) { rays_o[p * 3 + b] = o[b]; rays_d[p * 3 + b] = d[b]; }
        if (viewdirs != nullptr) {
            const float inv = 1.f / sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
            for (int b = 0; b < 3; ++b) viewdirs[p * 3 + b] = d[b] * inv;
        }
        // C:212-214: |d(row) - d(row+1)| * 2/sqrt(12).  For a pin-hole camera that row difference is the same vector
        // for every pixel, (K^-1 e_y) R; evaluating it in closed form avoids the cancellation of two O(1) directions
        // that differ by 1/f (an fp32 subtraction would carry 2e-4 relative error at f = 1500).
        if (radii != nullptr) radii[p] = radius;
    }
}

__global__ __launch_bounds__(256) void rays_aabb_kernel(const float* __restrict__ rays_o, float* __restrict__ rays_d, long n,
                                                        float bx0, float by0, float bz0, float bx1, float by1, float bz1,
                                                        float* __restrict__ near, float* __restrict__ far, unsigned char* __restrict__ mask) {
    const Box bx = grown_box(bx0, by0, bz0, bx1, by1, bz1);
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long)gridDim.x * blockDim.x) {
        const float o[3] = {rays_o[p * 3], rays_o[p * 3 + 1], rays_o[p * 3 + 2]};
        float d[3] = {rays_d[p * 3], rays_d[p * 3 + 1], rays_d[p * 3 + 2]};
        const int clamped = clamp_dir(d);
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (clamped & (1 << a)) rays_d[p * 3 + a] = 1e-5f;                           // C:238 mutates ray_d in place
        float tn, tf;
        const bool ok = ray_box(bx, o, d, tn, tf);
        mask[p] = ok ? 1 : 0;
        near[p] = tn;
        far[p] = tf;
    }
}

// ------------------------------------------------------------------------------------------ compacted frame rays
// One thread per pixel, 256 pixels per block, the SAME block partition in the count and the write pass.  The three launches are
// ordered by the stream only: no kernel waits on another workgroup, each ends by itself whatever the data.
constexpr int FR_BLOCK = 256;          // 4 waves of 64
constexpr int FR_SCAN = 1024;          // 16 waves of 64

struct PixelRay { float o[3], d[3], near, far; bool ok; };

__device__ __forceinline__ PixelRay pixel_ray(const Cam& c, const Box& bx, long p, long n, int W) {
    PixelRay r;
    r.ok = false;
    r.near = r.far = 0.f;
    camera_origin(c, r.o);
    r.d[0] = r.d[1] = r.d[2] = 0.f;
    if (p < n) {
        const int row = (int)(p / W), col = (int)(p % W);
        pixel_dir(c, (float)col, (float)row, r.o, r.d);
        clamp_dir(r.d);
        r.ok = ray_box(bx, r.o, r.d, r.near, r.far);
    }
    return r;
}

__global__ __launch_bounds__(FR_BLOCK) void frame_count_kernel(Cam c, Box bx, int H, int W, int* __restrict__ block_count) {
    __shared__ int wave_n[FR_BLOCK / 64];
    const long n = (long)H * W;
    const long p = (long)blockIdx.x * FR_BLOCK + threadIdx.x;
    const PixelRay r = pixel_ray(c, bx, p, n, W);
    const unsigned long long hit = __ballot(r.ok);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = __popcll(hit);
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
}

// Exclusive scan of the block counts IN PLACE by ONE workgroup of 1024 threads.  More than 1024 counts (a 1024 x 512 frame has 2048)
// are handled by LOOPING inside this workgroup, 1024 counts per pass with the running total carried in a register every thread
// holds -- not by a second level of workgroups, and not by any wait on another workgroup.
__global__ __launch_bounds__(FR_SCAN) void frame_scan_kernel(int* __restrict__ block_count, int nblk, int* __restrict__ count) {
    __shared__ int wave_tot[FR_SCAN / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < nblk; base += FR_SCAN) {
        const int i = base + (int)threadIdx.x;
        const int v = i < nblk ? block_count[i] : 0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < FR_SCAN / 64; ++w) {
            const int t = wave_tot[w];
            if (w < wave) before += t;
            total += t;
        }
        if (i < nblk) block_count[i] = (carry + before) + (incl - v);
        carry += total;
        __syncthreads();                       // wave_tot is rewritten by the next pass
    }
    if (threadIdx.x == 0) count[0] = carry;
}

__global__ __launch_bounds__(FR_BLOCK) void frame_write_kernel(Cam c, Box bx, int H, int W, const int* __restrict__ block_offset,
                                                               float* __restrict__ rays_o, float* __restrict__ rays_d,
                                                               float* __restrict__ near, float* __restrict__ far,
                                                               int* __restrict__ pix, int* __restrict__ slot) {
    __shared__ int wave_n[FR_BLOCK / 64];
    const long n = (long)H * W;
    const long p = (long)blockIdx.x * FR_BLOCK + threadIdx.x;
    const PixelRay r = pixel_ray(c, bx, p, n, W);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long hit = __ballot(r.ok);
    if (lane == 0) wave_n[wave] = __popcll(hit);
    __syncthreads();
    int before = block_offset[blockIdx.x];
#pragma unroll
    for (int w = 0; w < FR_BLOCK / 64; ++w)
        if (w < wave) before += wave_n[w];
    const long k = (long)before + __popcll(hit & ((1ull << lane) - 1ull));       // rank among the kept rays = position in nonzero()
    if (p < n) slot[p] = (r.ok && k < n) ? (int)k : -1;
    if (r.ok && k < n) {                                                          // k < count <= n = the capacity of the lists
#pragma unroll
        for (int b = 0; b < 3; ++b) { rays_o[k * 3 + b] = r.o[b]; rays_d[k * 3 + b] = r.d[b]; }
        near[k] = r.near;
        far[k] = r.far;
        pix[k] = (int)p;
    }
}

// rendered = full(bg); rendered[ray_mask] = rgb (M:610-612, :627) and to_8b_image (M:629, truncation), one thread per pixel
__global__ __launch_bounds__(256) void frame_paint_kernel(const int* __restrict__ slot, const float* __restrict__ rgb,
                                                          int count, const float* __restrict__ bg01, long n, float* __restrict__ out_f32,
                                                          unsigned char* __restrict__ out_u8) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int k = slot[p];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const float v = (k >= 0 && k < count) ? rgb[(long)k * 3 + b] : bg01[b];      // count = rows of rgb: never read past them
        if (out_f32 != nullptr) out_f32[p * 3 + b] = v;
        if (out_u8 != nullptr) {
            const float cl = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
            out_u8[p * 3 + b] = (unsigned char)(255.f * cl);
        }
    }
}

inline int grid_n(long n) { long b = (n + 255) / 256; return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b)); }

}  // namespace

extern "C" int hos_camera_rays(const float* Kinv9, const float* R9, const float* T3, int H, int W, float* rays_o, float* rays_d,
                               float* viewdirs, float* radii, hos_stream_t stream) {
    if (!Kinv9 || !R9 || !T3 || !rays_o || !rays_d || H < 2 || W < 1) return HOS_E_ARG;
    Cam c;
    for (int i = 0; i < 9; ++i) { c.Kinv[i] = Kinv9[i]; c.R[i] = R9[i]; }      // HOST pointers: 21 camera scalars by value
    for (int i = 0; i < 3; ++i) c.T[i] = T3[i];
    hipLaunchKernelGGL(camera_rays_kernel, dim3(grid_n((long)H * W)), dim3(256), 0, static_cast<hipStream_t>(stream), c, H, W,
                       rays_o, rays_d, viewdirs, radii);
    return hos_launch_status();
}

extern "C" int hos_rays_aabb(const float* rays_o, float* rays_d, int64_t n, const float* bounds6, float* near, float* far,
                             unsigned char* mask, hos_stream_t stream) {
    if (!rays_o || !rays_d || !bounds6 || !near || !far || !mask || n <= 0) return HOS_E_ARG;
    hipLaunchKernelGGL(rays_aabb_kernel, dim3(grid_n(n)), dim3(256), 0, static_cast<hipStream_t>(stream), rays_o, rays_d, (long)n,
                       bounds6[0], bounds6[1], bounds6[2], bounds6[3], bounds6[4], bounds6[5], near, far, mask);   // HOST pointer: 6 floats
    return hos_launch_status();
}

extern "C" int hos_frame_rays_compact(const float* Kinv9, const float* R9, const float* T3, const float* bounds6, int H, int W,
                                      float* rays_o, float* rays_d, float* near, float* far, int32_t* pix, int32_t* slot,
                                      int32_t* count, int32_t* ws, hos_stream_t stream) {
    if (!Kinv9 || !R9 || !T3 || !bounds6 || !rays_o || !rays_d || !near || !far || !pix || !slot || !count || !ws || H < 2 || W < 1)
        return HOS_E_ARG;
    const long n = (long)H * W;
    if (n > 0x7fffffffL - FR_BLOCK) return HOS_E_SHAPE;                           // pixel and list indices are int32
    Cam c;
    for (int i = 0; i < 9; ++i) { c.Kinv[i] = Kinv9[i]; c.R[i] = R9[i]; }      // HOST pointers: camera and box scalars by value
    for (int i = 0; i < 3; ++i) c.T[i] = T3[i];
    const Box bx = grown_box(bounds6[0], bounds6[1], bounds6[2], bounds6[3], bounds6[4], bounds6[5]);
    const int nblk = (int)((n + FR_BLOCK - 1) / FR_BLOCK);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(frame_count_kernel, dim3(nblk), dim3(FR_BLOCK), 0, s, c, bx, H, W, ws);
    hipLaunchKernelGGL(frame_scan_kernel, dim3(1), dim3(FR_SCAN), 0, s, ws, nblk, count);
    hipLaunchKernelGGL(frame_write_kernel, dim3(nblk), dim3(FR_BLOCK), 0, s, c, bx, H, W, ws, rays_o, rays_d, near, far, pix, slot);
    return hos_launch_status();
}

extern "C" int hos_frame_paint(const int32_t* slot, const float* rgb, int count, const float* bg01, int H, int W, float* out_f32,
                               unsigned char* out_u8, hos_stream_t stream) {
    if (!slot || !bg01 || (!out_f32 && !out_u8) || H < 1 || W < 1 || count < 0 || (count > 0 && !rgb)) return HOS_E_ARG;
    const long n = (long)H * W;
    hipLaunchKernelGGL(frame_paint_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), slot, rgb,
                       count, bg01, n, out_f32, out_u8);
    return hos_launch_status();
}

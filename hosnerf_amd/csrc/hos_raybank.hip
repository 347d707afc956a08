// Stage-1 ray bank on the device (1st_State-Conditional_Scene/src/data = `D:`).  The reference builds a HOST table of every
// unmasked ray of the training split (D:interface.py:105-205 `split_each` over D:ray_utils.py:34-139 `batchified_get_rays`,
// 44 bytes per ray) and gathers each batch from it in DataLoader workers.  Here the table is never materialised: the device keeps
// the 8-bit images, a camera table and, per image, the LIST of kept pixels; a ray is recomputed from its pixel when it is drawn.
//   hos_raybank_index    once per scene: per image the kept pixels (keep[p] != 0, keep = mask < 1) in pixel order -- the order of the
//                        reference's `_rays_o[masks_idx]` -- as int32 at a running int64 offset into one `pix` buffer, plus the
//                        per-image counts (= `bkgrays_sizes`).  Per-block counts, a scan by ONE workgroup, a write pass.
//   hos_raybank_gather   per step: ray r = (image id, rank k in that image's list) -> pixel pix[offset[img] + k] -> rays_o, rays_d,
//                        viewdirs, radii, times, target
//   hos_raybank_frame    the same per-pixel functions for the pixels [start, start + n) of ONE camera passed by value (whole test
//                        frames, render-path cameras); rays are not masked (`split_each_val`), the target is optional
// Per-pixel arithmetic (D:ray_utils.py:61-108): dir = ((col + 0.5 - cx) / fx, (row + 0.5 - cy) / fy, 1), d = R dir, rays_d = viewdirs =
// d / |d| (`viewdirs = rays_d; viewdirs /= norm` acts in place on the same array, :87-88), rays_o = the camera centre, radius =
// |d(row) - d(row + 1)| * 2 / sqrt(12) on the un-normalised directions.  HBM-bound on the outputs: 56 B per ray.
#include "hos_common.h"

namespace {

constexpr int RB_BLOCK = 256;          // 4 waves of 64, one pixel / ray per thread
constexpr int RB_SCAN = 1024;          // 16 waves of 64
constexpr int RB_CAM = 16;             // floats per camera: camera-to-world 3x4 row-major, fx, fy, cx, cy

struct BankCam { float m[12]; float fx, fy, cx, cy; };

__device__ __forceinline__ BankCam load_cam(const float* __restrict__ cams, int img) {
    BankCam c;
    const float* p = cams + (long)img * RB_CAM;
#pragma unroll
    for (int i = 0; i < 12; ++i) c.m[i] = p[i];
    c.fx = p[12]; c.fy = p[13]; c.cx = p[14]; c.cy = p[15];
    return c;
}

// D:ray_utils.py:61-88 for one pixel: the unit direction (rays_d and viewdirs are the same array in the reference)
__device__ __forceinline__ void bank_dir(const BankCam& c, int row, int col, float (&u)[3]) {
    const float x = (((float)col + 0.5f) - c.cx) / c.fx;
    const float y = (((float)row + 0.5f) - c.cy) / c.fy;
    float d[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = (x * c.m[r * 4 + 0] + y * c.m[r * 4 + 1]) + c.m[r * 4 + 2];       // "hwc, rc -> hwr", dir z = 1
    const float norm = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) u[r] = d[r] / norm;
}

// D:ray_utils.py:96-108.  d(row) - d(row + 1) = -(1 / fy) R e_y for EVERY pixel of a pin-hole camera (the last row repeats the row
// above, the same vector): evaluated in closed form per camera, as camera_rays_kernel (hos_rays.hip) does -- the subtraction of two
// O(1) directions that differ by 1 / f would carry 2e-4 relative error in fp32 at f = 1500.
__device__ __forceinline__ float bank_radius(const BankCam& c) {
    const float e0 = c.m[1] / c.fy, e1 = c.m[5] / c.fy, e2 = c.m[9] / c.fy;
    return sqrtf((e0 * e0 + e1 * e1) + e2 * e2) * 2.f / sqrtf(12.f);
}

struct RayOut { float* rays_o; float* rays_d; float* viewdirs; float* radii; float* times; float* target; };

// every output row of ray r; rgb == nullptr writes no target
__device__ __forceinline__ void store_ray(const RayOut& out, long r, const BankCam& c, int row, int col, float time,
                                          const unsigned char* __restrict__ rgb) {
    float u[3];
    bank_dir(c, row, col, u);
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        out.rays_o[r * 3 + b] = c.m[b * 4 + 3];
        out.rays_d[r * 3 + b] = u[b];
        out.viewdirs[r * 3 + b] = u[b];
    }
    out.radii[r] = bank_radius(c);
    out.times[r] = time;
    if (rgb != nullptr) {
#pragma unroll
        for (int b = 0; b < 3; ++b) out.target[r * 3 + b] = (float)rgb[b] / 255.f;       // == float32(u / 255.0) for all 256 values
    }
}

// ------------------------------------------------------------------------------------------ index: count / scan / write
// Block b of image i (blockIdx.x = i * nblk + b) owns the pixels [b * 256, b * 256 + 256) of that image; the SAME partition in
// the count and in the write pass.  The three launches are ordered by the stream only: no kernel waits on another workgroup.
__global__ __launch_bounds__(RB_BLOCK) void bank_count_kernel(const unsigned char* __restrict__ keep, long HW, int nblk,
                                                              int* __restrict__ block_count) {
    __shared__ int wave_n[RB_BLOCK / 64];
    const long img = blockIdx.x / nblk;
    const long p = (long)(blockIdx.x % nblk) * RB_BLOCK + threadIdx.x;
    const bool k = p < HW && keep[img * HW + p] != 0;
    const unsigned long long hit = __ballot(k);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = __popcll(hit);
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
}

// ONE workgroup: image by image, an exclusive scan of that image's block counts in place (1024 counts per pass, the running total
// in a register every thread holds, as frame_scan_kernel of hos_rays.hip), the image's count, and the running int64 offset of its
// list.  An image's count is at most H*W < 2^31; only the offsets need 64 bits.
__global__ __launch_bounds__(RB_SCAN) void bank_scan_kernel(int* __restrict__ block_count, int N, int nblk, int* __restrict__ counts,
                                                            int64_t* __restrict__ offsets) {
    __shared__ int wave_tot[RB_SCAN / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t running = 0;
    for (int img = 0; img < N; ++img) {
        int* bc = block_count + (long)img * nblk;
        int carry = 0;
        for (int base = 0; base < nblk; base += RB_SCAN) {
            const int i = base + (int)threadIdx.x;
            const int v = i < nblk ? bc[i] : 0;
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
            for (int w = 0; w < RB_SCAN / 64; ++w) {
                const int t = wave_tot[w];
                if (w < wave) before += t;
                total += t;
            }
            if (i < nblk) bc[i] = (carry + before) + (incl - v);
            carry += total;
            __syncthreads();                       // wave_tot is rewritten by the next pass
        }
        if (threadIdx.x == 0) { counts[img] = carry; offsets[img] = running; }
        running += carry;
    }
    if (threadIdx.x == 0) offsets[N] = running;
}

__global__ __launch_bounds__(RB_BLOCK) void bank_write_kernel(const unsigned char* __restrict__ keep, long HW, int nblk,
                                                              const int* __restrict__ block_offset,
                                                              const int64_t* __restrict__ offsets, int64_t cap,
                                                              int* __restrict__ pix) {
    __shared__ int wave_n[RB_BLOCK / 64];
    const long img = blockIdx.x / nblk;
    const long p = (long)(blockIdx.x % nblk) * RB_BLOCK + threadIdx.x;
    const bool k = p < HW && keep[img * HW + p] != 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long hit = __ballot(k);
    if (lane == 0) wave_n[wave] = __popcll(hit);
    __syncthreads();
    int before = block_offset[blockIdx.x];
#pragma unroll
    for (int w = 0; w < RB_BLOCK / 64; ++w)
        if (w < wave) before += wave_n[w];
    const int64_t at = offsets[img] + before + __popcll(hit & ((1ull << lane) - 1ull));     // rank among the image's kept pixels
    if (k && at >= 0 && at < cap) pix[at] = (int)p;                                               // cap = rows of pix: never write past them
}

// ------------------------------------------------------------------------------------------ per-step gather
__global__ __launch_bounds__(RB_BLOCK) void bank_gather_kernel(const float* __restrict__ cams, const float* __restrict__ times,
                                                               const unsigned char* __restrict__ images,
                                                               const int* __restrict__ pix, const int64_t* __restrict__ offsets,
                                                               const int* __restrict__ counts, const int* __restrict__ img_id,
                                                               const int* __restrict__ rank, long B, int N, int H, int W,
                                                               int64_t cap, RayOut out) {
    const long r = (long)blockIdx.x * RB_BLOCK + threadIdx.x;
    if (r >= B) return;
    const long HW = (long)H * W;
    const int img = img_id[r], k = rank[r];
    long p = -1;
    if (img >= 0 && img < N && k >= 0 && k < counts[img]) {
        const int64_t at = offsets[img] + k;
        if (at >= 0 && at < cap) p = pix[at];
    }
    if (p < 0 || p >= HW) {
        // an index outside the bank reads nothing; the row is NaN so that it cannot pass for a ray (the caller draws k < counts[img])
        const float q = __int_as_float(0x7fc00000);
#pragma unroll
        for (int b = 0; b < 3; ++b) { out.rays_o[r * 3 + b] = q; out.rays_d[r * 3 + b] = q; out.viewdirs[r * 3 + b] = q; out.target[r * 3 + b] = q; }
        out.radii[r] = q;
        out.times[r] = q;
        return;
    }
    const BankCam c = load_cam(cams, img);
    store_ray(out, r, c, (int)(p / W), (int)(p % W), times[img], images + ((long)img * HW + p) * 3);
}

// ------------------------------------------------------------------------------------------ a pixel range of one camera
__global__ __launch_bounds__(RB_BLOCK) void bank_frame_kernel(BankCam c, float time, int W, long start, long n,
                                                              const unsigned char* __restrict__ image, RayOut out) {
    const long r = (long)blockIdx.x * RB_BLOCK + threadIdx.x;
    if (r >= n) return;
    const long p = start + r;                                                  // the host checked start + n <= H * W
    store_ray(out, r, c, (int)(p / W), (int)(p % W), time, image != nullptr ? image + p * 3 : nullptr);
}

}  // namespace

extern "C" int hos_raybank_index(const unsigned char* keep, int N, int H, int W, int32_t* pix, int64_t cap, int32_t* counts,
                                 int64_t* offsets, int32_t* ws, hos_stream_t stream) {
    if (!keep || !pix || !counts || !offsets || !ws || N < 1 || H < 1 || W < 1 || cap < 0) return HOS_E_ARG;
    const long HW = (long)H * W;
    if (HW > 0x7fffffffL - RB_BLOCK) return HOS_E_SHAPE;                         // pixel indices are int32
    const long nblk = (HW + RB_BLOCK - 1) / RB_BLOCK;
    if (nblk * N > 0x7fffffffL) return HOS_E_SHAPE;                              // one workgroup per 256 pixels of the stack
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)(nblk * N);                                  // >= 1: N, H, W >= 1
    hipLaunchKernelGGL(bank_count_kernel, dim3(grid), dim3(RB_BLOCK), 0, s, keep, HW, (int)nblk, ws);
    hipLaunchKernelGGL(bank_scan_kernel, dim3(1), dim3(RB_SCAN), 0, s, ws, N, (int)nblk, counts, offsets);
    hipLaunchKernelGGL(bank_write_kernel, dim3(grid), dim3(RB_BLOCK), 0, s, keep, HW, (int)nblk, ws, offsets, cap, pix);
    return hos_launch_status();
}

extern "C" int hos_raybank_gather(const float* cams, const float* times, const unsigned char* images, const int32_t* pix,
                                  const int64_t* offsets, const int32_t* counts, const int32_t* img_id, const int32_t* rank,
                                  int64_t B, int N, int H, int W, int64_t cap, float* rays_o, float* rays_d, float* viewdirs,
                                  float* radii, float* times_out, float* target, hos_stream_t stream) {
    if (B < 0 || N < 1 || H < 1 || W < 1 || cap < 0) return HOS_E_ARG;
    if (B == 0) return HOS_OK;                                                   // nothing to launch
    if (!cams || !times || !images || !pix || !offsets || !counts || !img_id || !rank || !rays_o || !rays_d || !viewdirs || !radii ||
        !times_out || !target)
        return HOS_E_ARG;
    if ((long)H * W > 0x7fffffffL - RB_BLOCK) return HOS_E_SHAPE;
    const long nb = (B + RB_BLOCK - 1) / RB_BLOCK;
    if (nb > 0x7fffffffL) return HOS_E_SHAPE;
    const RayOut out{rays_o, rays_d, viewdirs, radii, times_out, target};
    hipLaunchKernelGGL(bank_gather_kernel, dim3((unsigned)nb), dim3(RB_BLOCK), 0, static_cast<hipStream_t>(stream), cams, times, images,
                       pix, offsets, counts, img_id, rank, (long)B, N, H, W, cap, out);
    return hos_launch_status();
}

extern "C" int hos_raybank_frame(const float* cam16, float time, int H, int W, int64_t start, int64_t n, const unsigned char* image,
                                 float* rays_o, float* rays_d, float* viewdirs, float* radii, float* times_out, float* target,
                                 hos_stream_t stream) {
    if (!cam16 || H < 1 || W < 1 || start < 0 || n < 0 || start + n > (int64_t)H * W) return HOS_E_ARG;
    if (n == 0) return HOS_OK;                                                   // nothing to launch
    if (!rays_o || !rays_d || !viewdirs || !radii || !times_out || (image != nullptr) != (target != nullptr)) return HOS_E_ARG;
    if ((long)H * W > 0x7fffffffL - RB_BLOCK) return HOS_E_SHAPE;
    BankCam c;
    for (int i = 0; i < 12; ++i) c.m[i] = cam16[i];                              // HOST pointer: the camera's 16 scalars by value
    c.fx = cam16[12]; c.fy = cam16[13]; c.cx = cam16[14]; c.cy = cam16[15];
    const RayOut out{rays_o, rays_d, viewdirs, radii, times_out, target};
    hipLaunchKernelGGL(bank_frame_kernel, dim3((unsigned)((n + RB_BLOCK - 1) / RB_BLOCK)), dim3(RB_BLOCK), 0,
                       static_cast<hipStream_t>(stream), c, time, W, (long)start, (long)n, image, out);
    return hos_launch_status();
}

// Mesh rasteriser (this build's addition; the reference has no counterpart): the meshes of hos_mesh.hip seen again through a frame's
// own camera, as the maps the renderer writes -- silhouette, depth, a shaded preview -- and a reduction that scores one set of maps
// against another.
//
//   hos_mesh_project    one thread per vertex: X_cam = R x + T, u = (K X_cam).x / X_cam.z, v = (K X_cam).y / X_cam.z, z = X_cam.z --
//                       the camera of pixel_dir (hos_rays.hip): pixel centres at integer coordinates, and with K's last row (0,0,1) the
//                       ray parameter t of a human ray IS the camera-space z.  xy = lrintf(256 u), lrintf(256 v): 1/256-pixel fixed point.
//   hos_raster_faces    one thread per triangle: exact integer coverage (64-bit edge functions, top-left rule, either orientation),
//                       perspective-correct depth, one 64-bit atomicMin per covered pixel on the key (bits(z) << 32) | face id
//   hos_raster_resolve  one thread per pixel: the winning face's barycentrics again -> face, depth, mask, rgb, normal, shaded
//   hos_frame_fit       counts and depth-difference sums of one set of maps against another: per-block partials in a fixed order, one
//                       final block, sums in double, no floating-point atomics
//
// The key: z > 0 is finite, positive floats order as their bit patterns, so the unsigned minimum is the nearest surface and, at equal
// depth, the lowest face id -- whatever the launch order.  An empty pixel is all ones (int64 -1), above every key.
// One thread per triangle fits marched meshes, whose triangles are a voxel across: a pixel or two (DESIGN.md quotes the measured
// boxes).  The loop of one triangle is over its pixel box clamped to the frame: at most H*W steps whatever the input.
#include "hos_common.h"

namespace {

constexpr int RS_BLOCK = 256;            // 4 waves of 64
constexpr int FIT_BLOCKS = 1024;         // most blocks of the fit's first pass = threads of its final block
constexpr int FIT_FINAL = 1024;
constexpr float RS_GUARD = 16384.f;      // |u|, |v| <= 2^14 pixels: |xy| <= 2^22, differences < 2^24, edge functions < 2^49

struct RsCam { float K[9]; float R[9]; float T[3]; };
struct RsView { float Kinv[9]; float R[9]; };

// ------------------------------------------------------------------------------------------ projection
__global__ __launch_bounds__(RS_BLOCK) void mesh_project_kernel(const float* __restrict__ vertices, long V, RsCam c, float z_near,
                                                                int* __restrict__ xy, float* __restrict__ z) {
    const long i = (long)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (i >= V) return;
    const float x = vertices[i * 3 + 0], y = vertices[i * 3 + 1], w = vertices[i * 3 + 2];
    float q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = ((c.R[a * 3 + 0] * x + c.R[a * 3 + 1] * y) + c.R[a * 3 + 2] * w) + c.T[a];      // R x + T
    const float px = (c.K[0] * q[0] + c.K[1] * q[1]) + c.K[2] * q[2];
    const float py = (c.K[3] * q[0] + c.K[4] * q[1]) + c.K[5] * q[2];
    const float u = px / q[2], v = py / q[2];
    // NaN fails every comparison: unusable
    const bool ok = q[2] > z_near && q[2] <= 3.402823466e38f && fabsf(u) <= RS_GUARD && fabsf(v) <= RS_GUARD;
    xy[i * 2 + 0] = ok ? (int)lrintf(256.f * u) : INT32_MIN;
    xy[i * 2 + 1] = ok ? (int)lrintf(256.f * v) : 0;
    z[i] = q[2];
}

// ------------------------------------------------------------------------------------------ one triangle on the screen
// The triangle after sign normalisation (area2 > 0: corners 1 and 2 swapped where the input's area is negative), with what coverage
// and interpolation need.  `ok` false: a corner index outside [0, V), an unusable corner or zero area.
struct ScreenTri {
    long long x[3], y[3];          // 1/256-pixel fixed point
    long long area2;               // > 0
    int bias[3];                   // 0 where edge i (opposite corner i) is a top or a left edge, else -1
    float iz[3];                   // 1 / z of the corners
    int v[3];                      // vertex ids, in the normalised order
    bool ok;
};

__device__ __forceinline__ ScreenTri load_tri(const int* __restrict__ xy, const float* __restrict__ z, const int* __restrict__ faces,
                                              long f, int V) {
    ScreenTri t;
    t.ok = false;
    t.area2 = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { t.x[k] = 0; t.y[k] = 0; t.bias[k] = 0; t.iz[k] = 0.f; t.v[k] = 0; }
    int id[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) id[k] = faces[f * 3 + k];
    if (id[0] < 0 || id[0] >= V || id[1] < 0 || id[1] >= V || id[2] < 0 || id[2] >= V) return t;
    int xi[3], yi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { xi[k] = xy[(long)id[k] * 2]; yi[k] = xy[(long)id[k] * 2 + 1]; }
    if (xi[0] == INT32_MIN || xi[1] == INT32_MIN || xi[2] == INT32_MIN) return t;
    const long long a2 = (long long)(xi[1] - xi[0]) * (yi[2] - yi[0]) - (long long)(yi[1] - yi[0]) * (xi[2] - xi[0]);
    if (a2 == 0) return t;
    const bool sw = a2 < 0;
    t.v[0] = id[0]; t.v[1] = sw ? id[2] : id[1]; t.v[2] = sw ? id[1] : id[2];
    t.x[0] = xi[0]; t.x[1] = sw ? xi[2] : xi[1]; t.x[2] = sw ? xi[1] : xi[2];
    t.y[0] = yi[0]; t.y[1] = sw ? yi[2] : yi[1]; t.y[2] = sw ? yi[1] : yi[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) t.iz[k] = 1.f / z[t.v[k]];
    t.area2 = a2 > 0 ? a2 : -a2;
    // edge i runs from corner i+1 to corner i+2; E(p) = dx (p.y - a.y) - dy (p.x - a.x) > 0 inside, its gradient (-dy, dx) points
    // inward: a left edge has dy < 0, a top edge dy == 0 and dx > 0 (y grows downward)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        const long long dx = t.x[b] - t.x[a], dy = t.y[b] - t.y[a];
        t.bias[k] = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : -1;
    }
    t.ok = true;
    return t;
}

// edge functions of the pixel centre (col, row); their sum is area2 exactly
__device__ __forceinline__ void edge_functions(const ScreenTri& t, int col, int row, long long (&e)[3]) {
    const long long px = (long long)col * 256, py = (long long)row * 256;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        e[k] = (t.x[b] - t.x[a]) * (py - t.y[a]) - (t.y[b] - t.y[a]) * (px - t.x[a]);
    }
}

__device__ __forceinline__ bool covered(const ScreenTri& t, const long long (&e)[3]) {
    return (e[0] + t.bias[0] >= 0) && (e[1] + t.bias[1] >= 0) && (e[2] + t.bias[2] >= 0);
}

// w_i = b_i / z_i with b_i = e_i / area2 in fp32, and the perspective-correct depth 1 / sum w_i
__device__ __forceinline__ float tri_depth(const ScreenTri& t, const long long (&e)[3], float (&w)[3]) {
    const float area = (float)t.area2;
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = ((float)e[k] / area) * t.iz[k];
    return 1.f / ((w[0] + w[1]) + w[2]);
}

// ------------------------------------------------------------------------------------------ coverage + depth test
__global__ __launch_bounds__(RS_BLOCK) void raster_faces_kernel(const int* __restrict__ xy, const float* __restrict__ z, int V,
                                                                const int* __restrict__ faces, long F, int face_base, int H, int W,
                                                                unsigned long long* __restrict__ zbuf, int* __restrict__ dropped) {
    const long f = (long)blockIdx.x * RS_BLOCK + threadIdx.x;
    const bool live = f < F;
    ScreenTri t;
    t.ok = false;
    if (live) t = load_tri(xy, z, faces, f, V);
    const bool drop = live && !t.ok;
    const unsigned long long db = __ballot(drop);
    if (db != 0ull && (int)(threadIdx.x & 63) == __ffsll((long long)db) - 1) atomicAdd(dropped, (int)__popcll(db));   // one per wave
    if (!live || !t.ok) return;
    long long xmin = min(t.x[0], min(t.x[1], t.x[2])), xmax = max(t.x[0], max(t.x[1], t.x[2]));
    long long ymin = min(t.y[0], min(t.y[1], t.y[2])), ymax = max(t.y[0], max(t.y[1], t.y[2]));
    // pixel centres sit at multiples of 256: ceil of the minimum, floor of the maximum (>> floors negative values too), then the frame
    const int c0 = (int)max((xmin + 255) >> 8, 0ll), c1 = (int)min(xmax >> 8, (long long)W - 1);
    const int r0 = (int)max((ymin + 255) >> 8, 0ll), r1 = (int)min(ymax >> 8, (long long)H - 1);
    const unsigned long long id = (unsigned long long)(unsigned)(face_base + (int)f);
    for (int row = r0; row <= r1; ++row)
        for (int col = c0; col <= c1; ++col) {
            long long e[3];
            edge_functions(t, col, row, e);
            if (!covered(t, e)) continue;
            float w[3];
            const float depth = tri_depth(t, e, w);
            const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | id;
            atomicMin(zbuf + ((long)row * W + col), key);
        }
}

// ------------------------------------------------------------------------------------------ resolve
__global__ __launch_bounds__(RS_BLOCK) void raster_resolve_kernel(const unsigned long long* __restrict__ zbuf, const int* __restrict__ xy,
                                                                  const float* __restrict__ z, int V, const int* __restrict__ faces,
                                                                  long F, int face_base, const float* __restrict__ vertices,
                                                                  const unsigned char* __restrict__ colors,
                                                                  const float* __restrict__ normals, RsView c, float bg0, float bg1,
                                                                  float bg2, int H, int W, int* __restrict__ face,
                                                                  float* __restrict__ depth, unsigned char* __restrict__ mask,
                                                                  float* __restrict__ rgb, float* __restrict__ normal,
                                                                  float* __restrict__ shaded) {
    const long p = (long)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (p >= (long)H * W) return;
    const unsigned long long key = zbuf[p];
    const float bg[3] = {bg0, bg1, bg2};
    if (key == ~0ull) {                                         // empty
        if (face != nullptr) face[p] = -1;
        if (depth != nullptr) depth[p] = 0.f;
        if (mask != nullptr) mask[p] = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (rgb != nullptr) rgb[p * 3 + k] = bg[k];
            if (normal != nullptr) normal[p * 3 + k] = 0.f;
            if (shaded != nullptr) shaded[p * 3 + k] = bg[k];
        }
        return;
    }
    const int id = (int)(unsigned)(key & 0xffffffffull);
    const long f = (long)id - face_base;
    if (id < 0 || f < 0 || f >= F) return;                      // another mesh won: untouched
    const float d = __uint_as_float((unsigned)(key >> 32));
    if (face != nullptr) face[p] = id;
    if (depth != nullptr) depth[p] = d;
    if (mask != nullptr) mask[p] = 1;
    if (rgb == nullptr && normal == nullptr && shaded == nullptr) return;
    const ScreenTri t = load_tri(xy, z, faces, f, V);
    if (!t.ok) return;                                          // cannot be: the face wrote this key
    const int row = (int)(p / W), col = (int)(p % W);
    long long e[3];
    edge_functions(t, col, row, e);
    float w[3];
    tri_depth(t, e, w);
    float colour[3] = {1.f, 1.f, 1.f};                          // absent colours: white
    if (colors != nullptr && (rgb != nullptr || shaded != nullptr)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float a0 = (float)colors[(long)t.v[0] * 3 + k], a1 = (float)colors[(long)t.v[1] * 3 + k], a2 = (float)colors[(long)t.v[2] * 3 + k];
            colour[k] = (((w[0] * a0 + w[1] * a1) + w[2] * a2) * d) / 255.f;
        }
    }
    if (rgb != nullptr) {
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb[p * 3 + k] = colour[k];
    }
    if (normal == nullptr && shaded == nullptr) return;
    float n[3];
    if (normals != nullptr) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            n[k] = ((w[0] * normals[(long)t.v[0] * 3 + k] + w[1] * normals[(long)t.v[1] * 3 + k]) + w[2] * normals[(long)t.v[2] * 3 + k]) * d;
    } else {
        // the face's geometric normal, in the INPUT's corner order (the normalised order may have swapped two corners)
        const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
        float a[3], b[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a[k] = vertices[(long)i1 * 3 + k] - vertices[(long)i0 * 3 + k];
            b[k] = vertices[(long)i2 * 3 + k] - vertices[(long)i0 * 3 + k];
        }
        n[0] = a[1] * b[2] - a[2] * b[1];
        n[1] = a[2] * b[0] - a[0] * b[2];
        n[2] = a[0] * b[1] - a[1] * b[0];
    }
    // scaled by the largest component first (vertex_normals_kernel): the squares of a tiny interpolant would underflow
    const float m = fmaxf(fmaxf(fabsf(n[0]), fabsf(n[1])), fabsf(n[2]));
    const bool ok = m > 0.f && m <= 3.402823466e38f;
    const float sx = n[0] / m, sy = n[1] / m, sz = n[2] / m;
    const float len = sqrtf((sx * sx + sy * sy) + sz * sz);                       // in [1, sqrt 3]
    n[0] = ok ? sx / len : 0.f;
    n[1] = ok ? sy / len : 0.f;
    n[2] = ok ? sz / len : 0.f;
    if (normal != nullptr) {
#pragma unroll
        for (int k = 0; k < 3; ++k) normal[p * 3 + k] = n[k];
    }
    if (shaded != nullptr) {
        // the pixel's ray direction in the mesh's space, R^T Kinv [col,row,1]: pixel_dir of hos_rays.hip, where T cancels against the origin
        float pc[3], dir[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) pc[a] = ((float)col * c.Kinv[a * 3 + 0] + (float)row * c.Kinv[a * 3 + 1]) + c.Kinv[a * 3 + 2];
#pragma unroll
        for (int b = 0; b < 3; ++b) dir[b] = (pc[0] * c.R[0 * 3 + b] + pc[1] * c.R[1 * 3 + b]) + pc[2] * c.R[2 * 3 + b];
        const float dl = sqrtf((dir[0] * dir[0] + dir[1] * dir[1]) + dir[2] * dir[2]);
        const float nd = ((n[0] * dir[0] + n[1] * dir[1]) + n[2] * dir[2]) / dl;
        const float shade = 0.3f + 0.7f * fabsf(nd);            // a head-light, two-sided
#pragma unroll
        for (int k = 0; k < 3; ++k) shaded[p * 3 + k] = colour[k] * shade;
    }
}

// ------------------------------------------------------------------------------------------ fit
struct FitAcc { long long a, b, ab; double sabs, sum, sq, mx; };

__device__ __forceinline__ FitAcc fit_zero() { return FitAcc{0, 0, 0, 0.0, 0.0, 0.0, 0.0}; }
__device__ __forceinline__ FitAcc fit_add(const FitAcc& x, const FitAcc& y) {
    return FitAcc{x.a + y.a, x.b + y.b, x.ab + y.ab, x.sabs + y.sabs, x.sum + y.sum, x.sq + y.sq, fmax(x.mx, y.mx)};
}
__device__ __forceinline__ FitAcc fit_shfl_xor(const FitAcc& x, int o) {
    return FitAcc{__shfl_xor(x.a, o, 64), __shfl_xor(x.b, o, 64), __shfl_xor(x.ab, o, 64), __shfl_xor(x.sabs, o, 64),
                  __shfl_xor(x.sum, o, 64), __shfl_xor(x.sq, o, 64), __shfl_xor(x.mx, o, 64)};
}
// the sum over a workgroup of NW waves, in a fixed order: xor tree inside each wave, then the waves ascending; valid in thread 0
template <int NW>
__device__ __forceinline__ FitAcc fit_block_sum(FitAcc v, FitAcc* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fit_add(v, fit_shfl_xor(v, o));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    FitAcc r = fit_zero();
    if (threadIdx.x == 0)
        for (int k = 0; k < NW; ++k) r = fit_add(r, sh[k]);
    return r;
}
__device__ __forceinline__ void fit_store(const FitAcc& r, long long* counts, double* sums) {
    counts[0] = r.a; counts[1] = r.b; counts[2] = r.ab;
    sums[0] = r.sabs; sums[1] = r.sum; sums[2] = r.sq; sums[3] = r.mx;
}

// ws: per block 3 counts then 4 doubles (7 words of 8 bytes)
__global__ __launch_bounds__(RS_BLOCK) void frame_fit_partial_kernel(const unsigned char* __restrict__ mask_a, const float* __restrict__ depth_a,
                                                                     const float* __restrict__ alpha_b, const float* __restrict__ depth_b,
                                                                     float tau, long n, long long* __restrict__ ws) {
    __shared__ FitAcc sh[RS_BLOCK / 64];
    FitAcc v = fit_zero();
    for (long i = (long)blockIdx.x * RS_BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * RS_BLOCK) {
        const bool a = mask_a[i] != 0, b = alpha_b[i] > tau;
        v.a += a; v.b += b;
        if (a && b) {
            v.ab += 1;
            if (depth_a != nullptr && depth_b != nullptr) {
                const double dz = (double)depth_a[i] - (double)depth_b[i];
                v.sabs += fabs(dz); v.sum += dz; v.sq += dz * dz; v.mx = fmax(v.mx, fabs(dz));
            }
        }
    }
    const FitAcc r = fit_block_sum<RS_BLOCK / 64>(v, sh);
    if (threadIdx.x == 0) fit_store(r, ws + (long)blockIdx.x * 7, reinterpret_cast<double*>(ws + (long)blockIdx.x * 7 + 3));
}

__global__ __launch_bounds__(FIT_FINAL) void frame_fit_final_kernel(const long long* __restrict__ ws, int nblk, long long* __restrict__ counts,
                                                                    double* __restrict__ sums) {
    __shared__ FitAcc sh[FIT_FINAL / 64];
    FitAcc v = fit_zero();
    if ((int)threadIdx.x < nblk) {
        const long long* w = ws + (long)threadIdx.x * 7;
        const double* d = reinterpret_cast<const double*>(w + 3);
        v = FitAcc{w[0], w[1], w[2], d[0], d[1], d[2], d[3]};
    }
    const FitAcc r = fit_block_sum<FIT_FINAL / 64>(v, sh);
    if (threadIdx.x == 0) fit_store(r, counts, sums);
}

inline bool frame_ok(int H, int W) { return H >= 1 && W >= 1 && (long)H * W <= 0x7fffffffL - RS_BLOCK; }

}  // namespace

extern "C" int hos_mesh_project(const float* vertices, int64_t V, const float* K9, const float* R9, const float* T3, float z_near,
                                int32_t* xy, float* z, hos_stream_t stream) {
    if (!K9 || !R9 || !T3 || V < 0 || !(z_near >= 0.f)) return HOS_E_ARG;
    if (V > 0x7fffffffL - RS_BLOCK) return HOS_E_SHAPE;                           // faces index vertices in int32
    if (V == 0) return HOS_OK;                                                     // nothing to launch
    if (!vertices || !xy || !z) return HOS_E_ARG;
    RsCam c;
    for (int i = 0; i < 9; ++i) { c.K[i] = K9[i]; c.R[i] = R9[i]; }               // HOST pointers: 21 camera scalars by value
    for (int i = 0; i < 3; ++i) c.T[i] = T3[i];
    hipLaunchKernelGGL(mesh_project_kernel, dim3((unsigned)((V + RS_BLOCK - 1) / RS_BLOCK)), dim3(RS_BLOCK), 0,
                       static_cast<hipStream_t>(stream), vertices, (long)V, c, z_near, xy, z);
    return hos_launch_status();
}

extern "C" int hos_raster_faces(const int32_t* xy, const float* z, int64_t V, const int32_t* faces, int64_t F, int face_base, int H, int W,
                                int64_t* zbuf, int32_t* dropped, hos_stream_t stream) {
    if (V < 0 || F < 0 || face_base < 0 || !zbuf || !dropped) return HOS_E_ARG;
    if (!frame_ok(H, W) || V > 0x7fffffffL - RS_BLOCK || F > 0x7fffffffL - RS_BLOCK - face_base) return HOS_E_SHAPE;   // ids are int32
    if (F == 0) return HOS_OK;                                                     // nothing to launch
    if (!faces || (V > 0 && (!xy || !z))) return HOS_E_ARG;
    hipLaunchKernelGGL(raster_faces_kernel, dim3((unsigned)((F + RS_BLOCK - 1) / RS_BLOCK)), dim3(RS_BLOCK), 0,
                       static_cast<hipStream_t>(stream), xy, z, (int)V, faces, (long)F, face_base, H, W,
                       reinterpret_cast<unsigned long long*>(zbuf), dropped);
    return hos_launch_status();
}

extern "C" int hos_raster_resolve(const int64_t* zbuf, const int32_t* xy, const float* z, int64_t V, const int32_t* faces, int64_t F,
                                  int face_base, const float* vertices, const unsigned char* colors, const float* normals,
                                  const float* Kinv9, const float* R9, const float* bg01, int H, int W, int32_t* face, float* depth,
                                  unsigned char* mask, float* rgb, float* normal, float* shaded, hos_stream_t stream) {
    if (V < 0 || F < 0 || face_base < 0 || !zbuf || !bg01) return HOS_E_ARG;
    if (!face && !depth && !mask && !rgb && !normal && !shaded) return HOS_E_ARG;
    if (!frame_ok(H, W) || V > 0x7fffffffL - RS_BLOCK || F > 0x7fffffffL - RS_BLOCK - face_base) return HOS_E_SHAPE;
    if (F == 0 || V == 0) return HOS_OK;                                           // nothing to launch
    if (!faces || !xy || !z) return HOS_E_ARG;
    if ((normal || shaded) && !normals && !vertices) return HOS_E_ARG;             // the geometric normal needs the positions
    if (shaded && (!Kinv9 || !R9)) return HOS_E_ARG;
    RsView c;
    for (int i = 0; i < 9; ++i) { c.Kinv[i] = Kinv9 ? Kinv9[i] : 0.f; c.R[i] = R9 ? R9[i] : 0.f; }     // HOST pointers
    const long n = (long)H * W;
    hipLaunchKernelGGL(raster_resolve_kernel, dim3((unsigned)((n + RS_BLOCK - 1) / RS_BLOCK)), dim3(RS_BLOCK), 0,
                       static_cast<hipStream_t>(stream), reinterpret_cast<const unsigned long long*>(zbuf), xy, z, (int)V, faces, (long)F,
                       face_base, vertices, colors, normals, c, bg01[0], bg01[1], bg01[2], H, W, face, depth, mask, rgb, normal, shaded);
    return hos_launch_status();
}

extern "C" int hos_frame_fit_blocks(void) { return FIT_BLOCKS; }

extern "C" int hos_frame_fit(const unsigned char* mask_a, const float* depth_a, const float* alpha_b, const float* depth_b, float tau,
                             int64_t n, int64_t* ws, int64_t* counts, double* sums, hos_stream_t stream) {
    if (n < 0 || !ws || !counts || !sums || !(tau == tau)) return HOS_E_ARG;
    if (n > 0 && (!mask_a || !alpha_b)) return HOS_E_ARG;
    if ((depth_a != nullptr) != (depth_b != nullptr)) return HOS_E_ARG;            // both depths or neither (silhouette only)
    const long want = (n + RS_BLOCK - 1) / RS_BLOCK;
    const int nblk = (int)(want > FIT_BLOCKS ? FIT_BLOCKS : want);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (nblk > 0)
        hipLaunchKernelGGL(frame_fit_partial_kernel, dim3(nblk), dim3(RS_BLOCK), 0, s, mask_a, depth_a, alpha_b, depth_b, tau, (long)n,
                           reinterpret_cast<long long*>(ws));
    hipLaunchKernelGGL(frame_fit_final_kernel, dim3(1), dim3(FIT_FINAL), 0, s, reinterpret_cast<const long long*>(ws), nblk,
                       reinterpret_cast<long long*>(counts), sums);
    return hos_launch_status();
}

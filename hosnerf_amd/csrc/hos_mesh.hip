// Canonical mesh (this build's addition; the reference has no counterpart): the field of one object state on a grid, and its isosurface.
//
//   hos_grid_points        the canonical positions of a range of grid vertices -- the rows the canonical MLP is evaluated on
//   hos_grid_alpha         alpha = mask * (1 - exp(-sigma h)) of that range into the whole-grid field (M:73-94 `_raw2outputs`: the alpha
//                          of a sample of length h under the motion-weight mask); mask = the K-channel sum of trilinear_zero, the device
//                          function and the expression of human_sample_warp_kernel (hos_human.hip) under identity bone transforms
//   hos_grid_warp          the frame mesh: the backward LBS (N:304-355) of a range of grid vertices of the frame's own box -> x_skel, mask,
//                          the rows the non-rigid chain and the canonical MLP are evaluated on (the renderer's warp, on a grid)
//   hos_grid_alpha_masked  hos_grid_alpha with that mask given (one kernel template, two instantiations)
//   hos_grid_alpha_density the background mesh (mesh.bkgd_field): alpha = 1 - exp(-density h), no mask, from the NeRF MLP's densities
//   hos_mesh_vertex_normals  per mesh vertex the normalised negative central difference of the trilinear field, spacing h
//   hos_march_tets_count   marching tetrahedra, count / scan: per 256-vertex block the mesh vertices its grid vertices own and the
//   hos_march_tets_write   triangles of its cells; one scan workgroup; the write pass at block offsets (as hos_raybank.hip)
//
// Grid: Nx x Ny x Nz vertices, vertex (ix,iy,iz) at origin + (float)i * h (grid_coord, the ONE expression), linear index
// u = (iz*Ny + iy)*Nx + ix.  Cell c0 = u (ix < Nx-1, ...) is cut into the 6 Kuhn tetrahedra {c0, c0+e_a, c0+e_a+e_b, c7}, one per
// permutation (a,b,c) of the axes in lexicographic order; corners are bit masks dx + 2dy + 4dz.  Every tetrahedron edge runs from a
// corner to a corner whose bits contain its own: from grid vertex v to v + d, d in 1..7; v owns it, family d - 1.  So thread u owns 7
// candidate mesh vertices and one cell, and reads the 8 corners of that cell: the edges it owns all start at corner 0.
// Streaming kernels: 8 field reads per vertex (7 of them neighbours' lines, L1 / L2 hits), 28 B of edge table written in the count
// pass; the write pass touches the table and the outputs near the surface only.
#include "hos_common.h"
#include "hos_trilinear.h"

namespace {

constexpr int MT_BLOCK = 256;          // 4 waves of 64, one grid vertex (= one cell, 7 owned edges) per thread
constexpr int MT_SCAN = 1024;          // 16 waves of 64: block counts scanned per pass of the one scan workgroup
constexpr int MT_KMAX = 32;            // bones (KMAX of hos_human.hip)

// Tetrahedron t: its four corners' bits, 3 bits each, vertex 0 lowest.  Permutations xyz, xzy, yxz, yzx, zxy, zyx.
__device__ __forceinline__ constexpr unsigned tet_corners(int t) {
    constexpr unsigned c[6] = {0u | (1u << 3) | (3u << 6) | (7u << 9), 0u | (1u << 3) | (5u << 6) | (7u << 9), 0u | (2u << 3) | (3u << 6) | (7u << 9),
                               0u | (2u << 3) | (6u << 6) | (7u << 9), 0u | (4u << 3) | (5u << 6) | (7u << 9), 0u | (4u << 3) | (6u << 6) | (7u << 9)};
    return c[t];
}
// Parity of the permutation: an odd tetrahedron is left-handed and swaps the last two corners of every triangle.
__device__ __forceinline__ constexpr bool tet_odd(int t) { return t == 1 || t == 2 || t == 5; }
// Tetrahedron edges 0..5 = (0,1) (1,2) (2,3) (0,2) (1,3) (0,3) as (lower, upper) tetrahedron vertex, 2 bits each.
constexpr unsigned EDGE_LO = 0u | (1u << 2) | (2u << 4) | (0u << 6) | (1u << 8) | (0u << 10);
constexpr unsigned EDGE_UP = 1u | (2u << 2) | (3u << 4) | (2u << 6) | (3u << 8) | (3u << 10);

// Triangles per inside mask (bit i = tetrahedron vertex i inside) of a RIGHT-handed tetrahedron, as tetrahedron edges: bits 0-1 the
// number of triangles, then 3 bits per corner.  The rule: ONE corner i inside (or one outside) -- the edges from i to the other
// three in ascending order, turned so that the normal points from the inside to the outside; TWO inside (i < j; k < l outside) --
// the quad (ik, il, jl, jk), turned the same way, cut along its diagonal ik-jl into (ik, il, jl) and (ik, jl, jk).
#define MT_TRI1(a, b, c) (1u | ((a) << 2) | ((b) << 5) | ((c) << 8))
#define MT_TRI2(a, b, c, d, e, f) (2u | ((a) << 2) | ((b) << 5) | ((c) << 8) | ((d) << 11) | ((e) << 14) | ((f) << 17))
__device__ const unsigned MT_TRI[16] = {
    0u,                    MT_TRI1(0u, 3u, 5u),   MT_TRI1(0u, 4u, 1u),   MT_TRI2(3u, 5u, 4u, 3u, 4u, 1u),
    MT_TRI1(3u, 1u, 2u),   MT_TRI2(0u, 2u, 5u, 0u, 1u, 2u), MT_TRI2(0u, 4u, 2u, 0u, 2u, 3u), MT_TRI1(5u, 4u, 2u),
    MT_TRI1(5u, 2u, 4u),   MT_TRI2(0u, 3u, 2u, 0u, 2u, 4u), MT_TRI2(0u, 2u, 1u, 0u, 5u, 2u), MT_TRI1(3u, 2u, 1u),
    MT_TRI2(3u, 1u, 4u, 3u, 4u, 5u), MT_TRI1(0u, 1u, 4u), MT_TRI1(0u, 5u, 3u),   0u};

struct MeshGrid { int Nx, Ny, Nz; float ox, oy, oz, h; };

__device__ __forceinline__ float grid_coord(float o, int i, float h) { return o + (float)i * h; }

// ------------------------------------------------------------------------------------------ the field on the grid
__global__ __launch_bounds__(MT_BLOCK) void grid_points_kernel(MeshGrid g, long first, long count, float* __restrict__ pts) {
    const long r = (long)blockIdx.x * MT_BLOCK + threadIdx.x;
    if (r >= count) return;
    const long u = first + r;
    const int ix = (int)(u % g.Nx), iy = (int)((u / g.Nx) % g.Ny), iz = (int)(u / ((long)g.Nx * g.Ny));
    pts[r * 3 + 0] = grid_coord(g.ox, ix, g.h);
    pts[r * 3 + 1] = grid_coord(g.oy, iy, g.h);
    pts[r * 3 + 2] = grid_coord(g.oz, iz, g.h);
}

// The backward LBS of one grid vertex per thread (N:304-355 `_sample_motion_fields`): the observed, body-frame position of the
// vertex -> x_skel and mask.  The K-loop and the division are lines 51-67 of human_sample_warp_kernel (hos_human.hip), COPIED: moved
// into a shared header they changed that kernel's instructions (commuted multiplies, inverted branches), so the renderer's kernel
// stays as it is and tests/test_gpu_frame_mesh.py holds the two bit-equal on the same points.
__global__ __launch_bounds__(MT_BLOCK) void grid_warp_kernel(const float* __restrict__ R, const float* __restrict__ T,
                                                             const float* __restrict__ vol, int V, int K,
                                                             const float* __restrict__ bbox_min, const float* __restrict__ bbox_scale,
                                                             MeshGrid g, long first, long count, float* __restrict__ x_skel,
                                                             float* __restrict__ mask) {
    __shared__ float sR[MT_KMAX * 9], sT[MT_KMAX * 3], sB[6];
    for (int i = threadIdx.x; i < K * 9; i += blockDim.x) sR[i] = R[i];
    for (int i = threadIdx.x; i < K * 3; i += blockDim.x) sT[i] = T[i];
    if (threadIdx.x < 3) { sB[threadIdx.x] = bbox_min[threadIdx.x]; sB[3 + threadIdx.x] = bbox_scale[threadIdx.x]; }
    __syncthreads();
    const long p = (long)blockIdx.x * MT_BLOCK + threadIdx.x;
    if (p >= count) return;
    const long u = first + p;
    const int ix = (int)(u % g.Nx), iy = (int)((u / g.Nx) % g.Ny), iz = (int)(u / ((long)g.Nx * g.Ny));
    const float px = grid_coord(g.ox, ix, g.h), py = grid_coord(g.oy, iy, g.h), pz = grid_coord(g.oz, iz, g.h);
    float wsum = 0.f, ax = 0.f, ay = 0.f, az = 0.f;
    const size_t V3 = (size_t)V * V * V;
    for (int i = 0; i < K; ++i) {
        const float* r = sR + i * 9;
        const float qx = (r[0] * px + r[1] * py + r[2] * pz) + sT[i * 3 + 0];              // N:319
        const float qy = (r[3] * px + r[4] * py + r[5] * pz) + sT[i * 3 + 1];
        const float qz = (r[6] * px + r[7] * py + r[8] * pz) + sT[i * 3 + 2];
        const float gx = (qx - sB[0]) * sB[3] - 1.f, gy = (qy - sB[1]) * sB[4] - 1.f, gz = (qz - sB[2]) * sB[5] - 1.f;
        const float w = trilinear_zero(vol + i * V3, V, gx, gy, gz);                        // N:322-324
        wsum += w;
        ax += w * qx; ay += w * qy; az += w * qz;                                           // N:333-338
    }
    const float den = fmaxf(wsum, 1e-4f);                                                   // N:339
    x_skel[p * 3] = ax / den; x_skel[p * 3 + 1] = ay / den; x_skel[p * 3 + 2] = az / den;
    mask[p] = wsum;
}

// MASK_GIVEN = false: hos_grid_alpha, the mask from the volume `vm` [>=K,V,V,V] at the vertex (the canonical mesh);
// MASK_GIVEN = true:  hos_grid_alpha_masked, the mask read from `vm` [count] (the frame mesh: what grid_warp_kernel wrote).
template <bool MASK_GIVEN>
__global__ __launch_bounds__(MT_BLOCK) void grid_alpha_kernel(const float* __restrict__ raw, const float* __restrict__ vm, int V, int K,
                                                              const float* __restrict__ bbox_min, const float* __restrict__ bbox_scale,
                                                              MeshGrid g, long first, long count, float* __restrict__ alpha,
                                                              float* __restrict__ rgb) {
    __shared__ float sB[6];
    if constexpr (!MASK_GIVEN) {
        if (threadIdx.x < 3) { sB[threadIdx.x] = bbox_min[threadIdx.x]; sB[3 + threadIdx.x] = bbox_scale[threadIdx.x]; }
        __syncthreads();
    }
    const long r = (long)blockIdx.x * MT_BLOCK + threadIdx.x;
    if (r >= count) return;
    const long u = first + r;
    const int ix = (int)(u % g.Nx), iy = (int)((u / g.Nx) % g.Ny), iz = (int)(u / ((long)g.Nx * g.Ny));
    float wsum = 0.f;
    if constexpr (MASK_GIVEN) {
        wsum = vm[r];
    } else {
        const float qx = grid_coord(g.ox, ix, g.h), qy = grid_coord(g.oy, iy, g.h), qz = grid_coord(g.oz, iz, g.h);
        const float gx = (qx - sB[0]) * sB[3] - 1.f, gy = (qy - sB[1]) * sB[4] - 1.f, gz = (qz - sB[2]) * sB[5] - 1.f;
        const size_t V3 = (size_t)V * V * V;
        for (int i = 0; i < K; ++i) wsum += trilinear_zero(vm + i * V3, V, gx, gy, gz);
    }
    const float sigma = raw[r * 4 + 3];
    const bool rim = ix == 0 || iy == 0 || iz == 0 || ix == g.Nx - 1 || iy == g.Ny - 1 || iz == g.Nz - 1;
    alpha[u] = rim ? 0.f : wsum * (1.f - expf(-sigma * g.h));        // the outermost layer is outside whatever the network says
    if (rgb != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[u * 3 + c] = raw[r * 4 + c];
    }
}

// The background mesh: no mask and no colour on the grid -- alpha = 1 - exp(-density h) of a range of vertices, 0 on the rim.
__global__ __launch_bounds__(MT_BLOCK) void grid_alpha_density_kernel(const float* __restrict__ density, MeshGrid g, long first, long count,
                                                                      float* __restrict__ alpha) {
    const long r = (long)blockIdx.x * MT_BLOCK + threadIdx.x;
    if (r >= count) return;
    const long u = first + r;
    const int ix = (int)(u % g.Nx), iy = (int)((u / g.Nx) % g.Ny), iz = (int)(u / ((long)g.Nx * g.Ny));
    const bool rim = ix == 0 || iy == 0 || iz == 0 || ix == g.Nx - 1 || iy == g.Ny - 1 || iz == g.Nz - 1;
    alpha[u] = rim ? 0.f : 1.f - expf(-density[r] * g.h);
}

// ------------------------------------------------------------------------------------------ marching tetrahedra
// What thread u knows of its cell: which of the 7 edges it owns carry a mesh vertex, and the inside bits of the 8 corners
// (corners outside the grid: outside; then the cell is not a cell and the edges towards them do not exist).
struct CellInfo {
    float f[8];            // corner values (0 where the corner is outside the grid)
    unsigned ins;          // bit cb: corner cb is inside
    unsigned emask;        // bit d-1: the edge u -> u + d exists and exactly one end is inside
    bool cell;             // all 8 corners exist
};

__device__ __forceinline__ CellInfo load_cell(const float* __restrict__ field, int Nx, int Ny, int Nz, long u, long N, float level) {
    CellInfo c;
    c.ins = 0u; c.emask = 0u; c.cell = false;
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) c.f[cb] = 0.f;
    if (u >= N) return c;
    const int ix = (int)(u % Nx), iy = (int)((u / Nx) % Ny), iz = (int)(u / ((long)Nx * Ny));
    unsigned have = 0u;
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) {
        const int dx = cb & 1, dy = (cb >> 1) & 1, dz = (cb >> 2) & 1;
        if (ix + dx < Nx && iy + dy < Ny && iz + dz < Nz) {
            c.f[cb] = field[u + dx + (long)dy * Nx + (long)dz * Nx * Ny];
            have |= 1u << cb;
            if (c.f[cb] > level) c.ins |= 1u << cb;                   // NaN and == level: outside
        }
    }
    c.cell = have == 0xffu;
    const unsigned in0 = c.ins & 1u;
#pragma unroll
    for (int d = 1; d < 8; ++d)
        if (((have >> d) & 1u) && ((c.ins >> d) & 1u) != in0) c.emask |= 1u << (d - 1);
    return c;
}

// inside mask of tetrahedron t (bit i = its vertex i) from the cell's corner bits
__device__ __forceinline__ unsigned tet_mask(unsigned ins, int t) {
    const unsigned cb = tet_corners(t);
    return ((ins >> (cb & 7u)) & 1u) | (((ins >> ((cb >> 3) & 7u)) & 1u) << 1) | (((ins >> ((cb >> 6) & 7u)) & 1u) << 2) |
           (((ins >> ((cb >> 9) & 7u)) & 1u) << 3);
}
__device__ __forceinline__ int tet_triangles(unsigned m) { return (m == 0u || m == 15u) ? 0 : (__popc(m) == 2 ? 2 : 1); }

// Ranks inside a wave from ballots: the mesh vertices (7 one-bit ballots, one per family) and the triangles (per tetrahedron
// "at least one" and "two") of the lanes below this one, and the wave's totals.
struct WaveRank { int v_before, v_total, f_before, f_total; };

__device__ __forceinline__ WaveRank wave_rank(const CellInfo& c, int lane) {
    const unsigned long long below = (1ull << lane) - 1ull;
    WaveRank w{0, 0, 0, 0};
#pragma unroll
    for (int fam = 0; fam < 7; ++fam) {
        const unsigned long long b = __ballot((c.emask >> fam) & 1u);
        w.v_before += __popcll(b & below);
        w.v_total += __popcll(b);
    }
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int n = c.cell ? tet_triangles(tet_mask(c.ins, t)) : 0;
        const unsigned long long b1 = __ballot(n >= 1), b2 = __ballot(n == 2);
        w.f_before += __popcll(b1 & below) + __popcll(b2 & below);
        w.f_total += __popcll(b1) + __popcll(b2);
    }
    return w;
}

// Block b owns the grid vertices [b * 256, b * 256 + 256): the SAME partition in the count and in the write pass.
__global__ __launch_bounds__(MT_BLOCK) void march_count_kernel(const float* __restrict__ field, int Nx, int Ny, int Nz, long N, float level,
                                                               int nblk, int* __restrict__ edge_slot, int* __restrict__ ws) {
    __shared__ int wave_v[MT_BLOCK / 64], wave_f[MT_BLOCK / 64];
    const long u = (long)blockIdx.x * MT_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const CellInfo c = load_cell(field, Nx, Ny, Nz, u, N, level);
    const WaveRank w = wave_rank(c, lane);
    if (lane == 0) { wave_v[wave] = w.v_total; wave_f[wave] = w.f_total; }
    __syncthreads();
    int before = w.v_before;
#pragma unroll
    for (int k = 0; k < MT_BLOCK / 64; ++k)
        if (k < wave) before += wave_v[k];
    if (u < N) {
#pragma unroll
        for (int fam = 0; fam < 7; ++fam)      // rank of edge (u, fam) among the block's mesh vertices, in (owner, family) order
            edge_slot[u * 7 + fam] = ((c.emask >> fam) & 1u) ? before + __popc(c.emask & ((1u << fam) - 1u)) : -1;
    }
    if (threadIdx.x == 0) {
        ws[blockIdx.x] = (wave_v[0] + wave_v[1]) + (wave_v[2] + wave_v[3]);
        ws[nblk + blockIdx.x] = (wave_f[0] + wave_f[1]) + (wave_f[2] + wave_f[3]);
    }
}

// ONE workgroup: the exclusive scan in place of the blocks' vertex counts, then of their triangle counts (1024 counts per pass, the
// running total in a register every thread holds, as bank_scan_kernel of hos_raybank.hip).  V <= 7 N < 2^31; the triangle total is
// carried in 64 bits and saturates at 2^31 - 1 (a field of noise on the largest grids), which the host refuses.
__global__ __launch_bounds__(MT_SCAN) void march_scan_kernel(int* __restrict__ ws, int nblk, int* __restrict__ counts) {
    __shared__ int wave_tot[MT_SCAN / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int which = 0; which < 2; ++which) {
        int* bc = ws + (long)which * nblk;
        long long carry = 0;
        for (int base = 0; base < nblk; base += MT_SCAN) {
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
            for (int k = 0; k < MT_SCAN / 64; ++k) {
                const int t = wave_tot[k];
                if (k < wave) before += t;
                total += t;
            }
            if (i < nblk) bc[i] = (int)min(carry + before + (incl - v), 0x7fffffffLL);
            carry += total;
            __syncthreads();                       // wave_tot is rewritten by the next pass
        }
        if (threadIdx.x == 0) counts[which] = (int)min(carry, 0x7fffffffLL);
    }
}

// mesh vertex id of edge `e` (0..5) of tetrahedron t of cell u: the edge's lower corner owns it
__device__ __forceinline__ int tet_edge_vertex(const int* __restrict__ edge_slot, const int* __restrict__ ws, long u, int Nx, long NxNy,
                                               unsigned corners, unsigned e) {
    const unsigned lo = (corners >> (3u * ((EDGE_LO >> (2u * e)) & 3u))) & 7u, up = (corners >> (3u * ((EDGE_UP >> (2u * e)) & 3u))) & 7u;
    const long owner = u + (lo & 1u) + (long)((lo >> 1) & 1u) * Nx + (long)((lo >> 2) & 1u) * NxNy;
    return ws[owner / MT_BLOCK] + edge_slot[owner * 7 + (long)(up - lo) - 1];
}

__global__ __launch_bounds__(MT_BLOCK) void march_write_kernel(const float* __restrict__ field, const float* __restrict__ rgb, MeshGrid g,
                                                               long N, float level, int nblk, const int* __restrict__ edge_slot,
                                                               const int* __restrict__ ws, int V, int F, float* __restrict__ vertices,
                                                               float* __restrict__ colors, int* __restrict__ faces) {
    __shared__ int wave_f[MT_BLOCK / 64];
    const long u = (long)blockIdx.x * MT_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Nx = g.Nx;
    const long NxNy = (long)g.Nx * g.Ny;
    const CellInfo c = load_cell(field, g.Nx, g.Ny, g.Nz, u, N, level);
    const WaveRank w = wave_rank(c, lane);
    if (lane == 0) wave_f[wave] = w.f_total;
    __syncthreads();
    // ---- the mesh vertices this grid vertex owns
    if (c.emask != 0u) {
        const int ix = (int)(u % g.Nx), iy = (int)((u / g.Nx) % g.Ny), iz = (int)(u / NxNy);
        const float px = grid_coord(g.ox, ix, g.h), py = grid_coord(g.oy, iy, g.h), pz = grid_coord(g.oz, iz, g.h);
        const int base = ws[blockIdx.x];
        const float fv = c.f[0];
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            if (!((c.emask >> (d - 1)) & 1u)) continue;
            const int id = base + edge_slot[u * 7 + (d - 1)];
            if (id < 0 || id >= V) continue;                                       // V = rows of vertices: never write past them
            const float fw = c.f[d];
            float t = (isfinite(fv) && isfinite(fw)) ? (level - fv) / (fw - fv) : 0.5f;
            if (!(t >= 0.f && t <= 1.f)) t = 0.5f;                                  // no output is ever non-finite
            const int dx = d & 1, dy = (d >> 1) & 1, dz = (d >> 2) & 1;
            vertices[(long)id * 3 + 0] = px + t * ((float)dx * g.h);
            vertices[(long)id * 3 + 1] = py + t * ((float)dy * g.h);
            vertices[(long)id * 3 + 2] = pz + t * ((float)dz * g.h);
            if (colors != nullptr) {
                const long q = u + dx + (long)dy * Nx + (long)dz * NxNy;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float cv = rgb[u * 3 + k], cw = rgb[q * 3 + k];
                    colors[(long)id * 3 + k] = cv + t * (cw - cv);
                }
            }
        }
    }
    // ---- the triangles of this cell
    if (!c.cell) return;
    long at = (long)ws[nblk + blockIdx.x] + w.f_before;
#pragma unroll
    for (int k = 0; k < MT_BLOCK / 64; ++k)
        if (k < wave) at += wave_f[k];
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const unsigned m = tet_mask(c.ins, t);
        const int n = tet_triangles(m);
        if (n == 0) continue;
        const unsigned tri = MT_TRI[m];
        for (int k = 0; k < n; ++k, ++at) {
            if (at >= F) continue;                                                  // F = rows of faces
            const unsigned e0 = (tri >> (2 + 9 * k)) & 7u, e1 = (tri >> (5 + 9 * k)) & 7u, e2 = (tri >> (8 + 9 * k)) & 7u;
            const int a = tet_edge_vertex(edge_slot, ws, u, Nx, NxNy, tet_corners(t), e0);
            const int b = tet_edge_vertex(edge_slot, ws, u, Nx, NxNy, tet_corners(t), tet_odd(t) ? e2 : e1);
            const int d = tet_edge_vertex(edge_slot, ws, u, Nx, NxNy, tet_corners(t), tet_odd(t) ? e1 : e2);
            faces[at * 3 + 0] = a; faces[at * 3 + 1] = b; faces[at * 3 + 2] = d;
        }
    }
}

// ------------------------------------------------------------------------------------------ vertex normals
// T(p): the trilinear interpolant of the whole-grid field at the position (x,y,z), in grid-index coordinates c = (p - origin) / h,
// zero outside the grid (a tap that is no grid vertex contributes nothing).  The weights and the tap order are trilinear_zero's; the
// grid is Nx x Ny x Nz, not cubic, and its coordinates are indices, not [-1,1] -- hence a function of its own.
__device__ __forceinline__ float trilinear_grid(const float* __restrict__ field, const MeshGrid& g, float x, float y, float z) {
    const float cx = (x - g.ox) / g.h, cy = (y - g.oy) / g.h, cz = (z - g.oz) / g.h;
    const float fx = floorf(cx), fy = floorf(cy), fz = floorf(cz);
    // NaN / huge coordinates: every tap out of range -> 0
    if (!(fx >= -1.f && fx <= (float)g.Nx && fy >= -1.f && fy <= (float)g.Ny && fz >= -1.f && fz <= (float)g.Nz)) return 0.f;
    const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
    const float wx1 = cx - fx, wy1 = cy - fy, wz1 = cz - fz;
    const float wx0 = (fx + 1.f) - cx, wy0 = (fy + 1.f) - cy, wz0 = (fz + 1.f) - cz;
    float out = 0.f;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int xi = x0 + dx, yi = y0 + dy, zi = z0 + dz;
                if (xi >= 0 && xi < g.Nx && yi >= 0 && yi < g.Ny && zi >= 0 && zi < g.Nz) {
                    const float w = (dx ? wx1 : wx0) * (dy ? wy1 : wy0) * (dz ? wz1 : wz0);
                    out += field[((long)zi * g.Ny + yi) * g.Nx + xi] * w;
                }
            }
    return out;
}

// One mesh vertex per thread: g_a = T(v + h e_a) - T(v - h e_a), n = -g / |g| (the field falls from the inside to the outside, so
// -g points outward, like the faces' orientation); (0,0,0) when g is 0 or not finite.  48 field reads per vertex, all within
// two cells of the vertex (L1 / L2 hits); no atomics, no adjacency: the result depends on the vertex and the field alone.
__global__ __launch_bounds__(MT_BLOCK) void vertex_normals_kernel(const float* __restrict__ field, MeshGrid g, const float* __restrict__ vertices,
                                                                  long V, float* __restrict__ normals) {
    const long i = (long)blockIdx.x * MT_BLOCK + threadIdx.x;
    if (i >= V) return;
    const float x = vertices[i * 3 + 0], y = vertices[i * 3 + 1], z = vertices[i * 3 + 2];
    const float gx = trilinear_grid(field, g, x + g.h, y, z) - trilinear_grid(field, g, x - g.h, y, z);
    const float gy = trilinear_grid(field, g, x, y + g.h, z) - trilinear_grid(field, g, x, y - g.h, z);
    const float gz = trilinear_grid(field, g, x, y, z + g.h) - trilinear_grid(field, g, x, y, z - g.h);
    // scaled by the largest component first: the squares of a gradient of 1e-20 (alpha in the tails of the mask) would underflow
    const float m = fmaxf(fmaxf(fabsf(gx), fabsf(gy)), fabsf(gz));
    const bool ok = m > 0.f && isfinite(gx) && isfinite(gy) && isfinite(gz);
    const float sx = gx / m, sy = gy / m, sz = gz / m;
    const float len = sqrtf((sx * sx + sy * sy) + sz * sz);                       // in [1, sqrt 3]
    normals[i * 3 + 0] = ok ? (-sx) / len : 0.f;
    normals[i * 3 + 1] = ok ? (-sy) / len : 0.f;
    normals[i * 3 + 2] = ok ? (-sz) / len : 0.f;
}

// HOS_OK and N = Nx*Ny*Nz, or HOS_E_SHAPE: a dimension below 2, or 7 N >= 2^31 - 256 (edge ids 7 u + family are int32)
int mesh_shape(int Nx, int Ny, int Nz, long* N) {
    if (Nx < 2 || Ny < 2 || Nz < 2) return HOS_E_SHAPE;
    const long limit = (0x7fffffffL - 256) / 7 + 1;          // N >= limit  <=>  7 N >= 2^31 - 256  (2^31 - 257 = 7 * 306783341 + 4)
    long n = (long)Nx * Ny;
    if (n >= limit) return HOS_E_SHAPE;
    n *= Nz;
    if (n >= limit) return HOS_E_SHAPE;
    *N = n;
    return HOS_OK;
}

}  // namespace

extern "C" int hos_grid_points(float ox, float oy, float oz, float h, int Nx, int Ny, int Nz, int64_t first, int64_t count, float* pts,
                               hos_stream_t stream) {
    if (!pts) return HOS_E_ARG;
    long N;
    if (int e = mesh_shape(Nx, Ny, Nz, &N)) return e;
    if (first < 0 || count < 0 || first > N || count > N - first) return HOS_E_ARG;
    if (count == 0) return HOS_OK;
    const MeshGrid g{Nx, Ny, Nz, ox, oy, oz, h};
    hipLaunchKernelGGL(grid_points_kernel, dim3((unsigned)((count + MT_BLOCK - 1) / MT_BLOCK)), dim3(MT_BLOCK), 0,
                       static_cast<hipStream_t>(stream), g, (long)first, (long)count, pts);
    return hos_launch_status();
}

extern "C" int hos_grid_alpha(const float* raw, const float* vol, int V, int K, const float* bbox_min, const float* bbox_scale, float ox,
                              float oy, float oz, float h, int Nx, int Ny, int Nz, int64_t first, int64_t count, float* alpha, float* rgb,
                              hos_stream_t stream) {
    if (!raw || !vol || !bbox_min || !bbox_scale || !alpha) return HOS_E_ARG;
    long N;
    if (int e = mesh_shape(Nx, Ny, Nz, &N)) return e;
    if (V < 1 || K < 1 || K > MT_KMAX) return HOS_E_SHAPE;
    if (first < 0 || count < 0 || first > N || count > N - first) return HOS_E_ARG;
    if (count == 0) return HOS_OK;
    const MeshGrid g{Nx, Ny, Nz, ox, oy, oz, h};
    hipLaunchKernelGGL(grid_alpha_kernel<false>, dim3((unsigned)((count + MT_BLOCK - 1) / MT_BLOCK)), dim3(MT_BLOCK), 0,
                       static_cast<hipStream_t>(stream), raw, vol, V, K, bbox_min, bbox_scale, g, (long)first, (long)count, alpha, rgb);
    return hos_launch_status();
}

extern "C" int hos_grid_warp(const float* R_b, const float* T_b, const float* vol, int V, int K, const float* bbox_min, const float* bbox_scale,
                             float ox, float oy, float oz, float h, int Nx, int Ny, int Nz, int64_t first, int64_t count, float* x_skel,
                             float* mask, hos_stream_t stream) {
    if (!R_b || !T_b || !vol || !bbox_min || !bbox_scale || !x_skel || !mask) return HOS_E_ARG;
    long N;
    if (int e = mesh_shape(Nx, Ny, Nz, &N)) return e;
    if (V < 1 || K < 1 || K > MT_KMAX) return HOS_E_SHAPE;
    if (first < 0 || count < 0 || first > N || count > N - first) return HOS_E_ARG;
    if (count == 0) return HOS_OK;
    const MeshGrid g{Nx, Ny, Nz, ox, oy, oz, h};
    hipLaunchKernelGGL(grid_warp_kernel, dim3((unsigned)((count + MT_BLOCK - 1) / MT_BLOCK)), dim3(MT_BLOCK), 0,
                       static_cast<hipStream_t>(stream), R_b, T_b, vol, V, K, bbox_min, bbox_scale, g, (long)first, (long)count, x_skel, mask);
    return hos_launch_status();
}

extern "C" int hos_grid_alpha_masked(const float* raw, const float* mask, float ox, float oy, float oz, float h, int Nx, int Ny, int Nz,
                                     int64_t first, int64_t count, float* alpha, float* rgb, hos_stream_t stream) {
    if (!raw || !mask || !alpha) return HOS_E_ARG;
    long N;
    if (int e = mesh_shape(Nx, Ny, Nz, &N)) return e;
    if (first < 0 || count < 0 || first > N || count > N - first) return HOS_E_ARG;
    if (count == 0) return HOS_OK;
    const MeshGrid g{Nx, Ny, Nz, ox, oy, oz, h};
    hipLaunchKernelGGL(grid_alpha_kernel<true>, dim3((unsigned)((count + MT_BLOCK - 1) / MT_BLOCK)), dim3(MT_BLOCK), 0,
                       static_cast<hipStream_t>(stream), raw, mask, 0, 0, (const float*)nullptr, (const float*)nullptr, g, (long)first,
                       (long)count, alpha, rgb);
    return hos_launch_status();
}

extern "C" int hos_grid_alpha_density(const float* density, float h, int Nx, int Ny, int Nz, int64_t first, int64_t count, float* alpha,
                                      hos_stream_t stream) {
    if (!density || !alpha) return HOS_E_ARG;
    long N;
    if (int e = mesh_shape(Nx, Ny, Nz, &N)) return e;
    if (first < 0 || count < 0 || first > N || count > N - first) return HOS_E_ARG;
    if (count == 0) return HOS_OK;
    const MeshGrid g{Nx, Ny, Nz, 0.f, 0.f, 0.f, h};
    hipLaunchKernelGGL(grid_alpha_density_kernel, dim3((unsigned)((count + MT_BLOCK - 1) / MT_BLOCK)), dim3(MT_BLOCK), 0,
                       static_cast<hipStream_t>(stream), density, g, (long)first, (long)count, alpha);
    return hos_launch_status();
}

extern "C" int hos_mesh_vertex_normals(const float* field, float ox, float oy, float oz, float h, int Nx, int Ny, int Nz,
                                       const float* vertices, int64_t V, float* normals, hos_stream_t stream) {
    if (!field || V < 0) return HOS_E_ARG;
    long N;
    if (int e = mesh_shape(Nx, Ny, Nz, &N)) return e;
    if (V > 7 * N) return HOS_E_SHAPE;                                            // a mesh of this grid has at most 7 vertices per grid vertex
    if (V == 0) return HOS_OK;                                                   // nothing to launch
    if (!vertices || !normals) return HOS_E_ARG;
    const MeshGrid g{Nx, Ny, Nz, ox, oy, oz, h};
    hipLaunchKernelGGL(vertex_normals_kernel, dim3((unsigned)((V + MT_BLOCK - 1) / MT_BLOCK)), dim3(MT_BLOCK), 0,
                       static_cast<hipStream_t>(stream), field, g, vertices, (long)V, normals);
    return hos_launch_status();
}

extern "C" int hos_march_tets_blocks(int Nx, int Ny, int Nz) {
    long N;
    if (int e = mesh_shape(Nx, Ny, Nz, &N)) return e;
    return (int)((N + MT_BLOCK - 1) / MT_BLOCK);
}

extern "C" int hos_march_tets_count(const float* field, int Nx, int Ny, int Nz, float level, int32_t* edge_slot, int32_t* ws,
                                    int32_t* counts, hos_stream_t stream) {
    if (!field || !edge_slot || !ws || !counts) return HOS_E_ARG;
    long N;
    if (int e = mesh_shape(Nx, Ny, Nz, &N)) return e;
    const int nblk = (int)((N + MT_BLOCK - 1) / MT_BLOCK);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(march_count_kernel, dim3((unsigned)nblk), dim3(MT_BLOCK), 0, s, field, Nx, Ny, Nz, N, level, nblk, edge_slot, ws);
    hipLaunchKernelGGL(march_scan_kernel, dim3(1), dim3(MT_SCAN), 0, s, ws, nblk, counts);
    return hos_launch_status();
}

extern "C" int hos_march_tets_write(const float* field, const float* rgb, int Nx, int Ny, int Nz, float level, float ox, float oy, float oz,
                                    float h, const int32_t* edge_slot, const int32_t* ws, int V, int F, float* vertices, float* colors,
                                    int32_t* faces, hos_stream_t stream) {
    if (!field || !edge_slot || !ws || V < 0 || F < 0) return HOS_E_ARG;
    long N;
    if (int e = mesh_shape(Nx, Ny, Nz, &N)) return e;
    if (V == 0 && F == 0) return HOS_OK;                                         // nothing to launch
    if (!vertices || !faces || (rgb != nullptr) != (colors != nullptr)) return HOS_E_ARG;
    const int nblk = (int)((N + MT_BLOCK - 1) / MT_BLOCK);
    const MeshGrid g{Nx, Ny, Nz, ox, oy, oz, h};
    hipLaunchKernelGGL(march_write_kernel, dim3((unsigned)nblk), dim3(MT_BLOCK), 0, static_cast<hipStream_t>(stream), field, rgb, g, N, level,
                       nblk, edge_slot, ws, V, F, vertices, colors, faces);
    return hos_launch_status();
}

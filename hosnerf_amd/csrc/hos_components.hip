// Mesh components (this build's addition; the reference has no counterpart): the connected pieces of a triangle mesh -- which piece
// a vertex belongs to, how many there are, what each one measures -- and the sub-mesh of the pieces the caller keeps.
//
//   hos_mesh_label_begin       label[v] = v, the four status words zeroed
//   hos_mesh_label_round       one round of min-label propagation: a hook launch (one thread per face) and a jump launch (one thread
//                              per vertex); the host repeats rounds until one leaves its `changed` word at 0
//   hos_mesh_component_ids     roots (label[r] == r) ranked in ascending order: count / scan / write, then one gather launch
//   hos_mesh_component_terms   per face its component and its area / volume terms in double; per component the vertex and face counts
//   hos_mesh_component_sums    per component the sums of the terms of its faces, in a fixed order
//   hos_mesh_compact_count     kept vertices / faces per 256-block, one scan workgroup -> (V', F')
//   hos_mesh_compact_write     the kept vertices (and colours, normals) gathered, then the kept faces renumbered
//
// What makes the labelling safe whatever the scheduling: a label is only ever LOWERED, and only by a device-scope integer atomicMin;
// a plain load of a label may be stale inside a launch (the per-XCD L2s and the L1s are not coherent with each other), which costs
// rounds and never the result; no kernel waits for, polls or hands data to another workgroup; no loop's trip count depends on
// another thread; the launch boundary is the only synchronisation.  Every value a label takes is a vertex id of its own component,
// and label[v] <= v.  A round that lowers nothing has read the true state, so then every face's three labels are equal and every
// label is a root: label[v] is the smallest vertex id of v's component, the one fixed point.
#include "hos_common.h"

namespace {

constexpr int MC_BLOCK = 256;          // 4 waves of 64, one vertex or one face per thread
constexpr int MC_SCAN = 1024;          // 16 waves of 64: block counts scanned per pass of the one scan workgroup
constexpr int MC_JUMPS = 2;            // pointer jumps per vertex and round

// words int32 [4]: the faces with a corner outside [0,V); `changed` of the even and of the odd rounds; the number of components
constexpr int W_INVALID = 0, W_CHANGED = 1, W_COUNT = 3;

__device__ __forceinline__ bool in_range(int i, int n) { return (unsigned)i < (unsigned)n; }

__global__ __launch_bounds__(MC_BLOCK) void label_begin_kernel(int V, int* __restrict__ label, int* __restrict__ words) {
    const int v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v < V) label[v] = v;
    if (v < 4) words[v] = 0;
}

// One face per thread: m = the smallest of the three labels read; every corner x, and the vertex its label names, is lowered to m.
// Round k reports into words[W_CHANGED + (k & 1)] and zeroes the word of round k + 1, which no thread of this round touches.
__global__ __launch_bounds__(MC_BLOCK) void label_hook_kernel(const int* __restrict__ faces, int F, int V, int round, int* label,
                                                              int* __restrict__ words) {
    const int f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f == 0) words[W_CHANGED + ((round + 1) & 1)] = 0;
    if (f >= F) return;
    const int x[3] = {faces[(long)f * 3 + 0], faces[(long)f * 3 + 1], faces[(long)f * 3 + 2]};
    if (!in_range(x[0], V) || !in_range(x[1], V) || !in_range(x[2], V)) {
        if (round == 0) atomicAdd(&words[W_INVALID], 1);
        return;
    }
    const int l[3] = {label[x[0]], label[x[1]], label[x[2]]};
    const int m = min(l[0], min(l[1], l[2]));
    bool changed = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (l[k] > m) changed |= atomicMin(&label[x[k]], m) > m;                     // l[k] == m: nothing to lower through this read
        if (l[k] > m && in_range(l[k], V)) changed |= atomicMin(&label[l[k]], m) > m;
    }
    if (changed) words[W_CHANGED + (round & 1)] = 1;
}

// One vertex per thread: label[v] := label[label[v]], MC_JUMPS times; the value carried to the next jump is what the atomic left.
__global__ __launch_bounds__(MC_BLOCK) void label_jump_kernel(int V, int round, int* label, int* __restrict__ words) {
    const int v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
    int l = label[v];
    bool changed = false;
#pragma unroll
    for (int j = 0; j < MC_JUMPS; ++j) {
        if (!in_range(l, V)) break;
        const int ll = label[l];
        if (ll < l) {
            changed |= atomicMin(&label[v], ll) > ll;
            l = ll;
        }
    }
    if (changed) words[W_CHANGED + (round & 1)] = 1;
}

// ------------------------------------------------------------------------------------------ count / scan / write
// Rank of this thread's flag among the block's flags, and the block's total (ballots per wave, wave totals through LDS).
__device__ __forceinline__ int block_rank(bool flag, int* wave_tot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) wave_tot[wave] = __popcll(b);
    __syncthreads();
    int before = __popcll(b & ((1ull << lane) - 1ull));
    total = 0;
#pragma unroll
    for (int k = 0; k < MC_BLOCK / 64; ++k) {
        if (k < wave) before += wave_tot[k];
        total += wave_tot[k];
    }
    __syncthreads();                               // wave_tot may be used again
    return before;
}

// ONE workgroup: the exclusive scan in place of ws[0, n0) and, with `two`, then of ws[n0, n0 + n1); totals into counts[0] and
// counts[1].  The shape of march_scan_kernel (hos_mesh.hip): 1024 counts per pass, the running total in a register
// every thread holds.  Every total is below 2^31: the entry points refuse V or F >= 2^31 - 256.
__global__ __launch_bounds__(MC_SCAN) void component_scan_kernel(int* __restrict__ ws, int n0, int n1, int two, int* __restrict__ counts) {
    __shared__ int wave_tot[MC_SCAN / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int which = 0; which < (two ? 2 : 1); ++which) {
        int* bc = ws + (which ? n0 : 0);
        const int n = which ? n1 : n0;
        int carry = 0;
        for (int base = 0; base < n; base += MC_SCAN) {
            const int i = base + (int)threadIdx.x;
            const int v = i < n ? bc[i] : 0;
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
            for (int k = 0; k < MC_SCAN / 64; ++k) {
                const int t = wave_tot[k];
                if (k < wave) before += t;
                total += t;
            }
            if (i < n) bc[i] = carry + before + (incl - v);
            carry += total;
            __syncthreads();                       // wave_tot is rewritten by the next pass
        }
        if (threadIdx.x == 0) counts[which] = carry;
    }
}

// ------------------------------------------------------------------------------------------ dense ids
__global__ __launch_bounds__(MC_BLOCK) void roots_count_kernel(const int* __restrict__ label, int V, int* __restrict__ ws) {
    __shared__ int wave_tot[MC_BLOCK / 64];
    const int v = blockIdx.x * MC_BLOCK + threadIdx.x;
    int total;
    block_rank(v < V && label[v] == v, wave_tot, total);
    if (threadIdx.x == 0) ws[blockIdx.x] = total;
}

// component[r] = rank of root r; the other vertices in the next launch (they read what this one wrote)
__global__ __launch_bounds__(MC_BLOCK) void roots_write_kernel(const int* __restrict__ label, int V, const int* __restrict__ ws,
                                                               int* __restrict__ component) {
    __shared__ int wave_tot[MC_BLOCK / 64];
    const int v = blockIdx.x * MC_BLOCK + threadIdx.x;
    const bool root = v < V && label[v] == v;
    int total;
    const int before = block_rank(root, wave_tot, total);
    if (root) component[v] = ws[blockIdx.x] + before;
}

__global__ __launch_bounds__(MC_BLOCK) void ids_gather_kernel(const int* __restrict__ label, int V, int* component) {
    const int v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
    const int l = label[v];
    if (l == v) return;
    component[v] = in_range(l, V) ? component[l] : -1;         // a converged labelling: l is a root, written by the launch before
}

// ------------------------------------------------------------------------------------------ per-component measures
// counts[c] += 1 for every active lane, with the lanes that share the first active lane's component folded into one add (a mesh's
// neighbouring ids mostly share a component): integer atomics, so the result is exact whatever the order.
__device__ __forceinline__ void count_into(unsigned long long* counts, int c, bool active) {
    const unsigned long long act = __ballot(active);
    if (act == 0ull) return;
    const int leader = __ffsll((long long)act) - 1;
    const int c0 = __shfl(c, leader, 64);
    const unsigned long long same = __ballot(active && c == c0);
    const int lane = threadIdx.x & 63;
    if (lane == leader) atomicAdd(&counts[c], (unsigned long long)__popcll(same));
    else if (active && c != c0) atomicAdd(&counts[c], 1ull);
}

__global__ __launch_bounds__(MC_BLOCK) void component_vertices_kernel(const int* __restrict__ component, int V, int C,
                                                                      unsigned long long* n_vertices) {
    const int v = blockIdx.x * MC_BLOCK + threadIdx.x;
    const int c = v < V ? component[v] : -1;
    count_into(n_vertices, c, in_range(c, C));
}

// Per face: area term |(b - a) x (c - a)| / 2 and volume term a . (b x c) / 6 of the fp32 vertices promoted to double
// (-ffp-contract=off: every product and sum is rounded on its own, in the order written here).
__global__ __launch_bounds__(MC_BLOCK) void component_terms_kernel(const float* __restrict__ vertices, const int* __restrict__ faces,
                                                                   const int* __restrict__ component, int V, int F, int C,
                                                                   int* __restrict__ face_component, double* __restrict__ terms,
                                                                   unsigned long long* n_faces) {
    const int f = blockIdx.x * MC_BLOCK + threadIdx.x;
    int fc = -1;
    if (f < F) {
        const int i0 = faces[(long)f * 3 + 0], i1 = faces[(long)f * 3 + 1], i2 = faces[(long)f * 3 + 2];
        double area = 0.0, volume = 0.0;
        if (in_range(i0, V) && in_range(i1, V) && in_range(i2, V)) {
            fc = component[i0];
            if (!in_range(fc, C)) fc = -1;
            const double ax = vertices[(long)i0 * 3 + 0], ay = vertices[(long)i0 * 3 + 1], az = vertices[(long)i0 * 3 + 2];
            const double bx = vertices[(long)i1 * 3 + 0], by = vertices[(long)i1 * 3 + 1], bz = vertices[(long)i1 * 3 + 2];
            const double cx = vertices[(long)i2 * 3 + 0], cy = vertices[(long)i2 * 3 + 1], cz = vertices[(long)i2 * 3 + 2];
            const double ux = bx - ax, uy = by - ay, uz = bz - az, wx = cx - ax, wy = cy - ay, wz = cz - az;
            const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
            area = sqrt((nx * nx + ny * ny) + nz * nz) / 2.0;
            const double mx = by * cz - bz * cy, my = bz * cx - bx * cz, mz = bx * cy - by * cx;
            volume = ((ax * mx + ay * my) + az * mz) / 6.0;
        }
        face_component[f] = fc;
        terms[(long)f * 2 + 0] = fc >= 0 ? area : 0.0;
        terms[(long)f * 2 + 1] = fc >= 0 ? volume : 0.0;
    }
    count_into(n_faces, fc, fc >= 0);
}

// One workgroup per component: thread t sums the terms of the faces order[start + t], order[start + t + 256], ... in that order, then
// a fixed tree over the 256 partial sums.  `order` is a stable sort of the face ids by component, so the order of every addition is
// a function of the mesh alone: two runs are bit-equal.
__global__ __launch_bounds__(MC_BLOCK) void component_sums_kernel(const double* __restrict__ terms, const long long* __restrict__ order,
                                                                  const long long* __restrict__ start, const long long* __restrict__ n_faces,
                                                                  long long F, double* __restrict__ area, double* __restrict__ volume) {
    __shared__ double sa[MC_BLOCK], sv[MC_BLOCK];
    const int c = blockIdx.x;
    const long long s = start[c], n = n_faces[c];
    double a = 0.0, v = 0.0;
    if (s >= 0 && n >= 0 && s <= F && n <= F - s) {
        for (long long i = threadIdx.x; i < n; i += MC_BLOCK) {
            const long long f = order[s + i];
            if (f < 0 || f >= F) continue;
            a += terms[f * 2 + 0];
            v += terms[f * 2 + 1];
        }
    }
    sa[threadIdx.x] = a; sv[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int o = MC_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { sa[threadIdx.x] += sa[threadIdx.x + o]; sv[threadIdx.x] += sv[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { area[c] = sa[0]; volume[c] = sv[0]; }
}

// ------------------------------------------------------------------------------------------ compaction
__device__ __forceinline__ bool vertex_kept(const unsigned char* __restrict__ keep, int C, const int* __restrict__ component, int V, int v) {
    if (v >= V) return false;
    const int c = component[v];
    return in_range(c, C) && keep[c] != 0;
}

// A face is kept iff it is valid, its component is kept and so is every corner (of a labelled mesh the last follows from the second)
__device__ __forceinline__ bool face_kept(const unsigned char* __restrict__ keep, int C, const int* __restrict__ component, int V,
                                          const int* __restrict__ faces, const int* __restrict__ face_component, int F, int f, int* corners) {
    if (f >= F) return false;
    const int fc = face_component[f];
    if (!in_range(fc, C) || keep[fc] == 0) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        corners[k] = faces[(long)f * 3 + k];
        if (!in_range(corners[k], V) || !vertex_kept(keep, C, component, V, corners[k])) return false;
    }
    return true;
}

// blocks [0, nbv): vertices; blocks [nbv, nbv + nbf): faces.  The SAME partition in the count and in the write launches.
__global__ __launch_bounds__(MC_BLOCK) void compact_count_kernel(const unsigned char* __restrict__ keep, int C, const int* __restrict__ component,
                                                                 int V, const int* __restrict__ faces, const int* __restrict__ face_component,
                                                                 int F, int nbv, int* __restrict__ ws) {
    __shared__ int wave_tot[MC_BLOCK / 64];
    int corners[3];
    const bool of_vertices = (int)blockIdx.x < nbv;
    const int i = (of_vertices ? (int)blockIdx.x : (int)blockIdx.x - nbv) * MC_BLOCK + threadIdx.x;
    const bool kept = of_vertices ? vertex_kept(keep, C, component, V, i) : face_kept(keep, C, component, V, faces, face_component, F, i, corners);
    int total;
    block_rank(kept, wave_tot, total);
    if (threadIdx.x == 0) ws[blockIdx.x] = total;
}

__global__ __launch_bounds__(MC_BLOCK) void compact_vertices_kernel(const unsigned char* __restrict__ keep, int C, const int* __restrict__ component,
                                                                    int V, const int* __restrict__ ws, const float* __restrict__ vertices,
                                                                    const unsigned char* __restrict__ colors, const float* __restrict__ normals,
                                                                    int Vout, int* __restrict__ new_id, float* __restrict__ out_vertices,
                                                                    unsigned char* __restrict__ out_colors, float* __restrict__ out_normals) {
    __shared__ int wave_tot[MC_BLOCK / 64];
    const int v = blockIdx.x * MC_BLOCK + threadIdx.x;
    const bool kept = vertex_kept(keep, C, component, V, v);
    int total;
    const int id = ws[blockIdx.x] + block_rank(kept, wave_tot, total);
    if (v >= V) return;
    const bool ok = kept && in_range(id, Vout);                                   // Vout = rows of the outputs: never write past them
    new_id[v] = ok ? id : -1;
    if (!ok) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out_vertices[(long)id * 3 + k] = vertices[(long)v * 3 + k];
        if (colors != nullptr) out_colors[(long)id * 3 + k] = colors[(long)v * 3 + k];
        if (normals != nullptr) out_normals[(long)id * 3 + k] = normals[(long)v * 3 + k];
    }
}

__global__ __launch_bounds__(MC_BLOCK) void compact_faces_kernel(const unsigned char* __restrict__ keep, int C, const int* __restrict__ component,
                                                                 int V, const int* __restrict__ faces, const int* __restrict__ face_component,
                                                                 int F, const int* __restrict__ ws_faces, const int* __restrict__ new_id,
                                                                 int Fout, int* __restrict__ out_faces) {
    __shared__ int wave_tot[MC_BLOCK / 64];
    int corners[3] = {0, 0, 0};
    const int f = blockIdx.x * MC_BLOCK + threadIdx.x;
    const bool kept = face_kept(keep, C, component, V, faces, face_component, F, f, corners);
    int total;
    const int at = ws_faces[blockIdx.x] + block_rank(kept, wave_tot, total);
    if (!kept || !in_range(at, Fout)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) out_faces[(long)at * 3 + k] = new_id[corners[k]];
}

constexpr int64_t MC_LIMIT = 0x80000000LL - 256;       // V, F below this: every id, block count and scanned total stays in int32

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + MC_BLOCK - 1) / MC_BLOCK); }

}  // namespace

extern "C" int hos_mesh_blocks(int64_t n) {
    if (n < 0) return HOS_E_ARG;
    if (n >= MC_LIMIT) return HOS_E_SHAPE;
    return (int)blocks_of(n);
}

extern "C" int hos_mesh_label_begin(int64_t V, int32_t* label, int32_t* words, hos_stream_t stream) {
    if (V < 0) return HOS_E_ARG;
    if (V >= MC_LIMIT) return HOS_E_SHAPE;
    if (V == 0) return HOS_OK;                                                   // nothing to launch
    if (!label || !words) return HOS_E_ARG;
    hipLaunchKernelGGL(label_begin_kernel, dim3(blocks_of(V)), dim3(MC_BLOCK), 0, static_cast<hipStream_t>(stream), (int)V, label, words);
    return hos_launch_status();
}

extern "C" int hos_mesh_label_round(const int32_t* faces, int64_t F, int64_t V, int round, int32_t* label, int32_t* words,
                                    hos_stream_t stream) {
    if (V < 0 || F < 0 || round < 0) return HOS_E_ARG;
    if (V >= MC_LIMIT || F >= MC_LIMIT) return HOS_E_SHAPE;
    if (V == 0 || F == 0) return HOS_OK;                                         // nothing to launch
    if (!faces || !label || !words) return HOS_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(label_hook_kernel, dim3(blocks_of(F)), dim3(MC_BLOCK), 0, s, faces, (int)F, (int)V, round, label, words);
    hipLaunchKernelGGL(label_jump_kernel, dim3(blocks_of(V)), dim3(MC_BLOCK), 0, s, (int)V, round, label, words);
    return hos_launch_status();
}

extern "C" int hos_mesh_component_ids(const int32_t* label, int64_t V, int32_t* component, int32_t* ws, int32_t* words,
                                      hos_stream_t stream) {
    if (V < 0) return HOS_E_ARG;
    if (V >= MC_LIMIT) return HOS_E_SHAPE;
    if (V == 0) return HOS_OK;                                                   // nothing to launch
    if (!label || !component || !ws || !words) return HOS_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned nb = blocks_of(V);
    hipLaunchKernelGGL(roots_count_kernel, dim3(nb), dim3(MC_BLOCK), 0, s, label, (int)V, ws);
    hipLaunchKernelGGL(component_scan_kernel, dim3(1), dim3(MC_SCAN), 0, s, ws, (int)nb, 0, 0, words + W_COUNT);
    hipLaunchKernelGGL(roots_write_kernel, dim3(nb), dim3(MC_BLOCK), 0, s, label, (int)V, ws, component);
    hipLaunchKernelGGL(ids_gather_kernel, dim3(nb), dim3(MC_BLOCK), 0, s, label, (int)V, component);
    return hos_launch_status();
}

extern "C" int hos_mesh_component_terms(const float* vertices, const int32_t* faces, const int32_t* component, int64_t V, int64_t F, int C,
                                        int32_t* face_component, double* terms, int64_t* n_vertices, int64_t* n_faces,
                                        hos_stream_t stream) {
    if (V < 0 || F < 0 || C < 0) return HOS_E_ARG;
    if (V >= MC_LIMIT || F >= MC_LIMIT || C > V) return HOS_E_SHAPE;
    if (V == 0 || C == 0) return HOS_OK;                                         // nothing to launch
    if (!component || !n_vertices || !n_faces) return HOS_E_ARG;
    if (F > 0 && (!vertices || !faces || !face_component || !terms)) return HOS_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(component_vertices_kernel, dim3(blocks_of(V)), dim3(MC_BLOCK), 0, s, component, (int)V, C,
                       reinterpret_cast<unsigned long long*>(n_vertices));
    if (F > 0)
        hipLaunchKernelGGL(component_terms_kernel, dim3(blocks_of(F)), dim3(MC_BLOCK), 0, s, vertices, faces, component, (int)V, (int)F, C,
                           face_component, terms, reinterpret_cast<unsigned long long*>(n_faces));
    return hos_launch_status();
}

extern "C" int hos_mesh_component_sums(const double* terms, const int64_t* order, const int64_t* start, const int64_t* n_faces, int64_t F,
                                       int C, double* area, double* volume, hos_stream_t stream) {
    if (F < 0 || C < 0) return HOS_E_ARG;
    if (F >= MC_LIMIT) return HOS_E_SHAPE;
    if (C == 0) return HOS_OK;                                                   // nothing to launch
    if (!start || !n_faces || !area || !volume || (F > 0 && (!terms || !order))) return HOS_E_ARG;
    hipLaunchKernelGGL(component_sums_kernel, dim3((unsigned)C), dim3(MC_BLOCK), 0, static_cast<hipStream_t>(stream), terms,
                       reinterpret_cast<const long long*>(order), reinterpret_cast<const long long*>(start),
                       reinterpret_cast<const long long*>(n_faces), (long long)F, area, volume);
    return hos_launch_status();
}

extern "C" int hos_mesh_compact_count(const unsigned char* keep, int C, const int32_t* component, int64_t V, const int32_t* faces,
                                      const int32_t* face_component, int64_t F, int32_t* ws, int32_t* counts, hos_stream_t stream) {
    if (V < 0 || F < 0 || C < 0) return HOS_E_ARG;
    if (V >= MC_LIMIT || F >= MC_LIMIT || C > V) return HOS_E_SHAPE;
    if (V == 0) return HOS_OK;                                                   // nothing to launch
    if (!keep || !component || !ws || !counts || C == 0 || (F > 0 && (!faces || !face_component))) return HOS_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned nbv = blocks_of(V), nbf = blocks_of(F);
    hipLaunchKernelGGL(compact_count_kernel, dim3(nbv + nbf), dim3(MC_BLOCK), 0, s, keep, C, component, (int)V, faces, face_component, (int)F,
                       (int)nbv, ws);
    hipLaunchKernelGGL(component_scan_kernel, dim3(1), dim3(MC_SCAN), 0, s, ws, (int)nbv, (int)nbf, 1, counts);
    return hos_launch_status();
}

extern "C" int hos_mesh_compact_write(const unsigned char* keep, int C, const int32_t* component, int64_t V, const int32_t* faces,
                                      const int32_t* face_component, int64_t F, const int32_t* ws, int32_t* new_id, const float* vertices,
                                      const unsigned char* colors, const float* normals, int64_t Vout, int64_t Fout, float* out_vertices,
                                      unsigned char* out_colors, float* out_normals, int32_t* out_faces, hos_stream_t stream) {
    if (V < 0 || F < 0 || C < 0 || Vout < 0 || Fout < 0 || Vout > V || Fout > F) return HOS_E_ARG;
    if (V >= MC_LIMIT || F >= MC_LIMIT || C > V) return HOS_E_SHAPE;
    if (V == 0 || Vout == 0) return HOS_OK;                                      // nothing to launch: a kept face has kept corners
    if (!keep || !component || !ws || !new_id || !vertices || !out_vertices || C == 0) return HOS_E_ARG;
    if (F > 0 && (!faces || !face_component || (Fout > 0 && !out_faces))) return HOS_E_ARG;
    if ((colors != nullptr) != (out_colors != nullptr) || (normals != nullptr) != (out_normals != nullptr)) return HOS_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned nbv = blocks_of(V), nbf = blocks_of(F);
    hipLaunchKernelGGL(compact_vertices_kernel, dim3(nbv), dim3(MC_BLOCK), 0, s, keep, C, component, (int)V, ws, vertices, colors, normals,
                       (int)Vout, new_id, out_vertices, out_colors, out_normals);
    if (Fout > 0)
        hipLaunchKernelGGL(compact_faces_kernel, dim3(nbf), dim3(MC_BLOCK), 0, s, keep, C, component, (int)V, faces, face_component, (int)F,
                           ws + nbv, new_id, (int)Fout, out_faces);
    return hos_launch_status();
}

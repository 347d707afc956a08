// The tracked mesh (this build's addition; the reference has no counterpart): the renderer's backward LBS INVERTED per point.
//
//   hos_warp_invert   for a target x* and a guess p0 per row: Newton's method on x_skel(p) = x*, x_skel the backward LBS of
//                     grid_warp_kernel (hos_mesh.hip; N:304-355) with its analytic Jacobian -> p, x_skel(p), mask(p), |x* - x_skel(p)|,
//                     a status and optionally the Jacobian, all evaluated at the returned p.  iters = 0 is a plain point warp.
//
// One row per thread, R_b / T_b / box in LDS as grid_warp_kernel keeps them, the row's state (p, 3 + 1 + 3 + 9 accumulators) in
// registers as scalars.  A gather out of the motion-weight volume (K * V^3 floats, 3.4 MB at K = 26, V = 32: L2-resident):
// (iterations + 1) * K * 8 loads per row, value and gradient from the same eight (trilinear_zero_grad).  fp32, no atomics, rows
// indexed in 64 bits; a row's result depends on that row's inputs alone, so two runs are bit-equal.
#include "hos_common.h"
#include "hos_trilinear_grad.h"

namespace {

constexpr int MT_BLOCK = 256;          // MT_BLOCK of hos_mesh.hip: 4 waves of 64, one row per thread
constexpr int MT_KMAX = 32;            // MT_KMAX of hos_mesh.hip: bones

enum { TRACK_CONVERGED = 0, TRACK_LIMIT = 1, TRACK_LOST = 2 };

__global__ __launch_bounds__(MT_BLOCK) void warp_invert_kernel(const float* __restrict__ target, const float* __restrict__ guess,
                                                               const float* __restrict__ R, const float* __restrict__ T,
                                                               const float* __restrict__ vol, int V, int K,
                                                               const float* __restrict__ bbox_min, const float* __restrict__ bbox_scale,
                                                               int iters, float tol, float max_step, long P, float* __restrict__ p_out,
                                                               float* __restrict__ x_skel, float* __restrict__ mask,
                                                               float* __restrict__ residual, int32_t* __restrict__ status,
                                                               float* __restrict__ jac) {
    __shared__ float sR[MT_KMAX * 9], sT[MT_KMAX * 3], sB[9];
    for (int i = threadIdx.x; i < K * 9; i += blockDim.x) sR[i] = R[i];
    for (int i = threadIdx.x; i < K * 3; i += blockDim.x) sT[i] = T[i];
    if (threadIdx.x < 3) {
        sB[threadIdx.x] = bbox_min[threadIdx.x];
        sB[3 + threadIdx.x] = bbox_scale[threadIdx.x];
        sB[6 + threadIdx.x] = bbox_scale[threadIdx.x] * (float)(V - 1) / 2.f;          // d(index) / d(q) per axis
    }
    __syncthreads();
    const long row = (long)blockIdx.x * MT_BLOCK + threadIdx.x;
    if (row >= P) return;
    const float tx = target[row * 3], ty = target[row * 3 + 1], tz = target[row * 3 + 2];
    float px = guess[row * 3], py = guess[row * 3 + 1], pz = guess[row * 3 + 2];
    const size_t V3 = (size_t)V * V * V;
    float x0, x1, x2, wsum, rn;
    float j00, j01, j02, j10, j11, j12, j20, j21, j22;
    int st;
    for (int it = 0;; ++it) {
        // x(p), W(p) as grid_warp_kernel forms them, and M = sum_i (q_i (x) g_i + w_i R_i), G = sum_i g_i, g_i = R_i^T grad_q w_i
        float ax = 0.f, ay = 0.f, az = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f;
        float m00 = 0.f, m01 = 0.f, m02 = 0.f, m10 = 0.f, m11 = 0.f, m12 = 0.f, m20 = 0.f, m21 = 0.f, m22 = 0.f;
        wsum = 0.f;
        for (int i = 0; i < K; ++i) {
            const float* r = sR + i * 9;
            const float qx = (r[0] * px + r[1] * py + r[2] * pz) + sT[i * 3 + 0];
            const float qy = (r[3] * px + r[4] * py + r[5] * pz) + sT[i * 3 + 1];
            const float qz = (r[6] * px + r[7] * py + r[8] * pz) + sT[i * 3 + 2];
            const float gx = (qx - sB[0]) * sB[3] - 1.f, gy = (qy - sB[1]) * sB[4] - 1.f, gz = (qz - sB[2]) * sB[5] - 1.f;
            float dx, dy, dz;
            const float w = trilinear_zero_grad(vol + i * V3, V, gx, gy, gz, &dx, &dy, &dz);
            dx *= sB[6]; dy *= sB[7]; dz *= sB[8];
            const float h0 = (r[0] * dx + r[3] * dy) + r[6] * dz;
            const float h1 = (r[1] * dx + r[4] * dy) + r[7] * dz;
            const float h2 = (r[2] * dx + r[5] * dy) + r[8] * dz;
            wsum += w;
            ax += w * qx; ay += w * qy; az += w * qz;
            g0 += h0; g1 += h1; g2 += h2;
            m00 += qx * h0 + w * r[0]; m01 += qx * h1 + w * r[1]; m02 += qx * h2 + w * r[2];
            m10 += qy * h0 + w * r[3]; m11 += qy * h1 + w * r[4]; m12 += qy * h2 + w * r[5];
            m20 += qz * h0 + w * r[6]; m21 += qz * h1 + w * r[7]; m22 += qz * h2 + w * r[8];
        }
        const float den = fmaxf(wsum, 1e-4f);
        x0 = ax / den; x1 = ay / den; x2 = az / den;
        if (wsum > 1e-4f) {                      // below the clamp the denominator is a constant: dx/dp = M / 1e-4
            m00 -= x0 * g0; m01 -= x0 * g1; m02 -= x0 * g2;
            m10 -= x1 * g0; m11 -= x1 * g1; m12 -= x1 * g2;
            m20 -= x2 * g0; m21 -= x2 * g1; m22 -= x2 * g2;
        }
        j00 = m00 / den; j01 = m01 / den; j02 = m02 / den;
        j10 = m10 / den; j11 = m11 / den; j12 = m12 / den;
        j20 = m20 / den; j21 = m21 / den; j22 = m22 / den;
        const float rx = tx - x0, ry = ty - x1, rz = tz - x2;
        rn = sqrtf((rx * rx + ry * ry) + rz * rz);
        if (!(isfinite(rx) && isfinite(ry) && isfinite(rz)) || !(wsum > 1e-4f)) { st = TRACK_LOST; break; }
        if (rn <= tol) { st = TRACK_CONVERGED; break; }
        if (it == iters) { st = TRACK_LIMIT; break; }
        const float c00 = j11 * j22 - j12 * j21, c01 = j10 * j22 - j12 * j20, c02 = j10 * j21 - j11 * j20;
        const float det = (j00 * c00 - j01 * c01) + j02 * c02;
        if (!(fabsf(det) > 1e-12f)) { st = TRACK_LOST; break; }
        float d0 = ((c00 * rx + (j02 * j21 - j01 * j22) * ry) + (j01 * j12 - j02 * j11) * rz) / det;
        float d1 = (((j12 * j20 - j10 * j22) * rx + (j00 * j22 - j02 * j20) * ry) + (j02 * j10 - j00 * j12) * rz) / det;
        float d2 = ((c02 * rx + (j01 * j20 - j00 * j21) * ry) + (j00 * j11 - j01 * j10) * rz) / det;
        const float dn = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
        if (dn > max_step) { const float s = max_step / dn; d0 *= s; d1 *= s; d2 *= s; }
        px += d0; py += d1; pz += d2;
    }
    p_out[row * 3] = px; p_out[row * 3 + 1] = py; p_out[row * 3 + 2] = pz;
    x_skel[row * 3] = x0; x_skel[row * 3 + 1] = x1; x_skel[row * 3 + 2] = x2;
    mask[row] = wsum;
    residual[row] = rn;
    status[row] = st;
    if (jac) {
        float* j = jac + row * 9;
        j[0] = j00; j[1] = j01; j[2] = j02; j[3] = j10; j[4] = j11; j[5] = j12; j[6] = j20; j[7] = j21; j[8] = j22;
    }
}

}  // namespace

extern "C" int hos_warp_invert(const float* target, const float* guess, const float* R_b, const float* T_b, const float* vol, int V, int K,
                               const float* bbox_min, const float* bbox_scale, int iters, float tol, float max_step, int64_t P,
                               float* p_out, float* x_skel, float* mask, float* residual, int32_t* status, float* jac,
                               hos_stream_t stream) {
    if (!target || !guess || !R_b || !T_b || !vol || !bbox_min || !bbox_scale || !p_out || !x_skel || !mask || !residual || !status)
        return HOS_E_ARG;
    if (P <= 0 || iters < 0 || !(tol > 0.f) || !(max_step > 0.f)) return HOS_E_ARG;
    if (V < 2 || K < 1 || K > MT_KMAX) return HOS_E_SHAPE;
    if (P > (int64_t)MT_BLOCK * 2147483647LL) return HOS_E_SHAPE;
    hipLaunchKernelGGL(warp_invert_kernel, dim3((unsigned)((P + MT_BLOCK - 1) / MT_BLOCK)), dim3(MT_BLOCK), 0,
                       static_cast<hipStream_t>(stream), target, guess, R_b, T_b, vol, V, K, bbox_min, bbox_scale, iters, tol, max_step,
                       (long)P, p_out, x_skel, mask, residual, status, jac);
    return hos_launch_status();
}

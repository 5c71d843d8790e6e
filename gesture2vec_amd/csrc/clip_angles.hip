// clip_angles.hip -- joint angles from generated clips: the arithmetic every make_bvh of the reference runs between the decoder's
// 3x3 matrices and pymo's inverse_transform (inference_Autoencoder.py:584-592, inference_text2embedding_GENEA.py:602-612,
// save_clustered_fast.py:180-188).
//   g2v_rotmat_to_euler     (N, 9 J) un-normalised 3x3 matrices -> (N, 3 J) intrinsic "ZXY" angles in degrees
//                           (scipy's Rotation.from_matrix(...).as_euler("ZXY", degrees=True), in either of its two behaviours)
//   g2v_smoothing_spline    (B, F, Cn) -> (B, F, Cn): de Boor's cubic smoothing spline along F at the knots
//                           (csaps.csaps(x, y, x, smooth=p) with uniform x = scipy's make_smoothing_spline(x, y, lam=(1-p)/p)(x))
//
// Conversion: one matrix per lane, float64 arithmetic from the float32 entries, one rounding on output.  36 B in, 12 B out per
// matrix; nothing is shared between lanes, no LDS.  G2V_ROT_PROCRUSTES first replaces the matrix by its orthogonal polar factor
// (the nearest rotation: det > 0 keeps it proper) by Higham's scaled Newton iteration X <- (g X + X^-T / g) / 2,
// g = sqrt(|X^-1|_F / |X|_F), X^-T = cof(X) / det(X): quadratic, at most ROT_NEWTON_MAX steps, stopped once a step moves X by
// less than 1e-13 in the Frobenius norm (the step after that would move it by about the square of that).  Then Markley's
// quaternion from the largest of m00, m11, m22, trace (the first on ties, as numpy's argmax), normalised; then the angles from the
// quaternion as scipy computes them (Bernardes & Viollet): X = 2 atan2(|(c, d)|, |(a, b)|) - pi/2, which keeps full precision at
// X = +-90 degrees where an arcsine of a matrix entry loses half the digits; within 1e-7 rad of the lock Y = 0 exactly and Z takes
// the combined rotation.
//
// Spline: with n = F - 2 and p = smooth, (6 (1-p) Q^T Q + p R) u = Q^T y, out = y - 6 (1-p) Q u; Q (F, n) has the columns
// (1, -2, 1), so the matrix is the pentadiagonal Toeplitz matrix (a2, a1, a0, a1, a2) = 6 (1-p) (1, -4, 6, -4, 1) + p (0, 1, 4, 1, 0):
// the same for every channel of every clip.
//   1. spline_factor_kernel: its L D L^T of bandwidth 2 in float64, once per call, by one lane (a serial chain of n steps of a few
//      FMAs and one division): per row i the triple (1 / d_i, e_i = L[i][i-1], f_i = L[i][i-2]), 3 n doubles at the workspace's start.
//   2. spline_sweep_kernel: one lane per (clip, channel).  Forward: z_i = (y_i - 2 y_i+1 + y_i+2) - e_i z_i-1 - f_i z_i-2 from three
//      rolling inputs; w_i = z_i / d_i goes to the workspace as float64, laid out (n, B Cn) so that a wavefront's 64 columns are 512
//      contiguous bytes.  Backward: u_i = w_i - e_i+1 u_i+1 - f_i+2 u_i+2, and out[t] = y[t] - 6 (1-p) (u_t - 2 u_t-1 + u_t-2) at
//      t = i + 2 needs only the three youngest u: it is written on the way down, u itself is never stored.  Both loops run in
//      blocks of SP_BLK steps whose loads (y, w and the factor's triples, none of which depends on the recurrence) are issued one
//      block ahead of the two dependent FMAs per step.  A lane reads only its own column and the shared factor: the same input
//      gives the same bits and a clip's bits do not depend on the batch.  In place (out == y) is safe: the forward pass writes
//      only the workspace, the backward pass loads y[t] before it stores out[t] (y and out are not __restrict__: the compiler
//      keeps that order), and no other lane touches the element.
//   Bytes per element: y read twice (8), w written and read (16), out written (4).
#include <math.h>

#include "common.hpp"

namespace g2v {
namespace {

constexpr int ROT_NEWTON_MAX = 48;          // scaled Newton reaches 1e-16 in <= 9 steps at condition 1e16; the cap only bounds the loop
constexpr double ROT_NEWTON_STOP2 = 1e-26;  // square of the Frobenius step below which the iterate is taken
constexpr double ROT_LOCK = 1e-7;           // scipy's gimbal-lock window, rad
constexpr int SP_MAX_F = 1 << 20;
constexpr int SP_BLK = 4;

__device__ __forceinline__ double det3(const double* m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

__device__ __forceinline__ void cof3(const double* m, double* c) {          // cofactor matrix: m^-T = c / det
  c[0] = m[4] * m[8] - m[5] * m[7];
  c[1] = m[5] * m[6] - m[3] * m[8];
  c[2] = m[3] * m[7] - m[4] * m[6];
  c[3] = m[2] * m[7] - m[1] * m[8];
  c[4] = m[0] * m[8] - m[2] * m[6];
  c[5] = m[1] * m[6] - m[0] * m[7];
  c[6] = m[1] * m[5] - m[2] * m[4];
  c[7] = m[2] * m[3] - m[0] * m[5];
  c[8] = m[0] * m[4] - m[1] * m[3];
}

__device__ __forceinline__ void nearest_rotation(double* m) {
  for (int it = 0; it < ROT_NEWTON_MAX; ++it) {
    double c[9];
    cof3(m, c);
    const double det = m[0] * c[0] + m[1] * c[1] + m[2] * c[2];
    double nm = 0.0, nc = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      nm += m[k] * m[k];
      nc += c[k] * c[k];
    }
    const double g = sqrt(sqrt(nc / nm) / fabs(det));       // |X^-1|_F = |cof|_F / |det|
    const double a = 0.5 * g, b = 0.5 / (g * det);
    double step2 = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const double x = a * m[k] + b * c[k];
      step2 += (x - m[k]) * (x - m[k]);
      m[k] = x;
    }
    if (!(step2 > ROT_NEWTON_STOP2)) break;                  // (also leaves on NaN)
  }
}

__global__ __launch_bounds__(256) void rotmat_to_euler_kernel(const float* __restrict__ frames, float* __restrict__ angles,
                                                              int64_t* __restrict__ bad, int64_t M, int method) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= M) return;
  const float* src = frames + idx * 9;
  float* dst = angles + idx * 3;
  double m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = (double)src[k];
  if (!(det3(m) > 0.0)) {                                    // zero, reflection, or a NaN entry
    const float qnan = __builtin_nanf("");
    dst[0] = qnan;
    dst[1] = qnan;
    dst[2] = qnan;
    atomicAdd(reinterpret_cast<unsigned long long*>(bad), 1ull);
    return;
  }
  if (method == G2V_ROT_PROCRUSTES) nearest_rotation(m);
  // Markley: (x, y, z, w) of the branch with the largest of m00, m11, m22, trace
  const double tr = m[0] + m[4] + m[8];
  int choice = 0;
  double best = m[0];
  if (m[4] > best) { choice = 1; best = m[4]; }
  if (m[8] > best) { choice = 2; best = m[8]; }
  if (tr > best) choice = 3;
  double qx, qy, qz, qw;
  if (choice == 0) {
    qx = 1.0 - tr + 2.0 * m[0]; qy = m[3] + m[1]; qz = m[6] + m[2]; qw = m[7] - m[5];
  } else if (choice == 1) {
    qy = 1.0 - tr + 2.0 * m[4]; qz = m[7] + m[5]; qx = m[1] + m[3]; qw = m[2] - m[6];
  } else if (choice == 2) {
    qz = 1.0 - tr + 2.0 * m[8]; qx = m[2] + m[6]; qy = m[5] + m[7]; qw = m[3] - m[1];
  } else {
    qx = m[7] - m[5]; qy = m[2] - m[6]; qz = m[3] - m[1]; qw = 1.0 + tr;
  }
  const double inv = 1.0 / sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
  qx *= inv; qy *= inv; qz *= inv; qw *= inv;
  // intrinsic ZXY = extrinsic y, x, z: (i, j, k) = (1, 0, 2), an odd permutation (sign -1)
  const double a = qw - qx, b = qy - qz, c = qx + qw, d = -qz - qy;
  const double pi = 3.14159265358979323846;
  const double second = 2.0 * atan2(hypot(c, d), hypot(a, b));           // X + pi/2 in [0, pi]
  const double half_sum = atan2(b, a), half_diff = atan2(d, c);
  double Z, Y;
  if (fabs(second) <= ROT_LOCK) {                // X = -90 degrees
    Y = 0.0;
    Z = -2.0 * half_sum;
  } else if (fabs(second - pi) <= ROT_LOCK) {    // X = +90 degrees
    Y = 0.0;
    Z = -2.0 * half_diff;
  } else {
    Y = half_sum - half_diff;
    Z = -(half_sum + half_diff);
  }
  double X = second - 0.5 * pi;
  if (Z < -pi) Z += 2.0 * pi; else if (Z > pi) Z -= 2.0 * pi;
  if (Y < -pi) Y += 2.0 * pi; else if (Y > pi) Y -= 2.0 * pi;
  const double deg = 180.0 / pi;
  dst[0] = (float)(Z * deg);
  dst[1] = (float)(X * deg);
  dst[2] = (float)(Y * deg);
}

// fac[3 i + 0..2] = 1 / d_i, e_i, f_i of the L D L^T of the n x n pentadiagonal Toeplitz matrix (a2, a1, a0, a1, a2)
__global__ __launch_bounds__(64) void spline_factor_kernel(double* __restrict__ fac, int n, double a0, double a1, double a2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double d1 = 0.0, d2 = 0.0, e1 = 0.0;       // d_i-1, d_i-2, e_i-1
  double r1 = 0.0, r2 = 0.0;                 // their reciprocals
  for (int i = 0; i < n; ++i) {
    const double f = i >= 2 ? a2 * r2 : 0.0;
    const double e = i >= 1 ? (a1 - f * e1 * d2) * r1 : 0.0;
    const double dd = a0 - e * e * d1 - f * f * d2;
    const double r = 1.0 / dd;
    fac[3 * (int64_t)i + 0] = r;
    fac[3 * (int64_t)i + 1] = e;
    fac[3 * (int64_t)i + 2] = f;
    d2 = d1; r2 = r1;
    d1 = dd; r1 = r;
    e1 = e;
  }
}

// one lane per column col = b Cn + c; element (b, t, c) of y / out is at (b F + t) Cn + c; w (n, ncol)
__global__ __launch_bounds__(64) void spline_sweep_kernel(const float* y, float* out, const double* __restrict__ fac,
                                                          double* __restrict__ w, int F, int Cn, int64_t ncol, double k6) {
  const int64_t col = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (col >= ncol) return;
  const int64_t b = col / Cn;
  const int64_t base = b * (int64_t)F * Cn + (col - b * Cn);             // element (b, 0, c)
  const float* yc = y + base;
  float* oc = out + base;
  double* wc = w + col;
  const int n = F - 2;
  // ---- forward substitution and the diagonal ----
  {
    double y0 = (double)yc[0], y1 = (double)yc[Cn];                      // y_i, y_i+1
    double z1 = 0.0, z2 = 0.0;                                           // z_i-1, z_i-2
    float ny[SP_BLK];
    double nf[SP_BLK][3];
#pragma unroll
    for (int k = 0; k < SP_BLK; ++k) {
      const int i = k < n ? k : n - 1;                                   // (clamped: a block past the end re-reads the last row)
      ny[k] = yc[(int64_t)(i + 2) * Cn];
      nf[k][0] = fac[3 * (int64_t)i]; nf[k][1] = fac[3 * (int64_t)i + 1]; nf[k][2] = fac[3 * (int64_t)i + 2];
    }
    for (int i0 = 0; i0 < n; i0 += SP_BLK) {
      float cy[SP_BLK];
      double cf[SP_BLK][3];
#pragma unroll
      for (int k = 0; k < SP_BLK; ++k) {
        cy[k] = ny[k];
        cf[k][0] = nf[k][0]; cf[k][1] = nf[k][1]; cf[k][2] = nf[k][2];
      }
#pragma unroll
      for (int k = 0; k < SP_BLK; ++k) {                                 // the next block's loads, ahead of this block's chain
        int i = i0 + SP_BLK + k;
        i = i < n ? i : n - 1;
        ny[k] = yc[(int64_t)(i + 2) * Cn];
        nf[k][0] = fac[3 * (int64_t)i]; nf[k][1] = fac[3 * (int64_t)i + 1]; nf[k][2] = fac[3 * (int64_t)i + 2];
      }
#pragma unroll
      for (int k = 0; k < SP_BLK; ++k) {
        const int i = i0 + k;
        if (i < n) {
          const double y2 = (double)cy[k];
          const double rhs = (y0 - 2.0 * y1) + y2;
          const double z = fma(-cf[k][2], z2, fma(-cf[k][1], z1, rhs));
          wc[(int64_t)i * ncol] = z * cf[k][0];
          z2 = z1; z1 = z;
          y0 = y1; y1 = y2;
        }
      }
    }
  }
  // ---- back substitution, out on the way down ----
  {
    double u1 = 0.0, u2 = 0.0;                                           // u_i+1, u_i+2
    double nw[SP_BLK], ne[SP_BLK], nfv[SP_BLK];
    float ny[SP_BLK];
    auto load = [&](int i, double& wv, double& ev, double& fv, float& yv) {
      const int ic = i > 0 ? i : 0;
      wv = wc[(int64_t)ic * ncol];
      ev = ic + 1 < n ? fac[3 * (int64_t)(ic + 1) + 1] : 0.0;            // e_i+1, f_i+2: zero past the last row
      fv = ic + 2 < n ? fac[3 * (int64_t)(ic + 2) + 2] : 0.0;
      yv = yc[(int64_t)(ic + 2) * Cn];
    };
#pragma unroll
    for (int k = 0; k < SP_BLK; ++k) load(n - 1 - k, nw[k], ne[k], nfv[k], ny[k]);
    for (int i0 = n - 1; i0 >= 0; i0 -= SP_BLK) {
      double cw[SP_BLK], ce[SP_BLK], cfv[SP_BLK];
      float cy[SP_BLK];
#pragma unroll
      for (int k = 0; k < SP_BLK; ++k) {
        cw[k] = nw[k]; ce[k] = ne[k]; cfv[k] = nfv[k]; cy[k] = ny[k];
      }
#pragma unroll
      for (int k = 0; k < SP_BLK; ++k) load(i0 - SP_BLK - k, nw[k], ne[k], nfv[k], ny[k]);
#pragma unroll
      for (int k = 0; k < SP_BLK; ++k) {
        const int i = i0 - k;
        if (i >= 0) {
          const double u = fma(-cfv[k], u2, fma(-ce[k], u1, cw[k]));
          oc[(int64_t)(i + 2) * Cn] = (float)((double)cy[k] - k6 * ((u2 - 2.0 * u1) + u));
          u2 = u1; u1 = u;
        }
      }
    }
    // u1 = u_0, u2 = u_1: rows 1 and 0 of Q u
    const double ya = (double)yc[Cn], yb = (double)yc[0];
    oc[Cn] = (float)(ya - k6 * (u2 - 2.0 * u1));
    oc[0] = (float)(yb - k6 * u1);
  }
}

}  // namespace
}  // namespace g2v

using namespace g2v;

extern "C" int g2v_rotmat_to_euler(const float* frames, float* angles, int64_t* bad, int64_t N, int J, int method,
                                   g2v_stream_t stream) {
  G2V_REQUIRE(frames && angles && bad, "null pointer");
  G2V_REQUIRE(N >= 1 && J >= 1, "N < 1 or J < 1");
  G2V_REQUIRE(method == G2V_ROT_MARKLEY || method == G2V_ROT_PROCRUSTES, "method is neither G2V_ROT_MARKLEY nor G2V_ROT_PROCRUSTES");
  G2V_REQUIRE(N <= (((int64_t)1 << 31) - 1) * 256 / J, "N * J matrices exceed the grid");
  const int64_t M = N * J;
  hipLaunchKernelGGL(rotmat_to_euler_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, frames, angles, bad, M,
                     method);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

extern "C" size_t g2v_smoothing_spline_workspace(int B, int F, int Cn) {
  if (B < 1 || Cn < 1 || F < 3 || F > SP_MAX_F || (int64_t)B * Cn >= ((int64_t)1 << 31)) return 0;
  const size_t n = (size_t)F - 2;
  return (3 * n + n * (size_t)B * (size_t)Cn) * sizeof(double);
}

extern "C" int g2v_smoothing_spline(const float* y, float* out, double smooth, int B, int F, int Cn, void* workspace,
                                    size_t workspace_bytes, g2v_stream_t stream) {
  G2V_REQUIRE(y && out, "null pointer");
  G2V_REQUIRE(B >= 1 && F >= 2 && Cn >= 1, "B < 1, F < 2 or Cn < 1");
  G2V_REQUIRE(smooth >= 0.0 && smooth <= 1.0, "smooth outside [0, 1]");          // (false for NaN)
  if (F > SP_MAX_F || (int64_t)B * Cn >= ((int64_t)1 << 31)) {
    set_error("g2v_smoothing_spline: F = %d, B * Cn = %lld: the kernels hold F <= %d and B * Cn < 2^31", F, (long long)B * Cn, SP_MAX_F);
    return G2V_ERR_UNSUPPORTED;
  }
  const size_t need = g2v_smoothing_spline_workspace(B, F, Cn);
  if (need > 0) {
    G2V_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "workspace is null or not 8-byte aligned");
    if (workspace_bytes < need) {
      set_error("g2v_smoothing_spline: workspace of %zu bytes, %zu needed", workspace_bytes, need);
      return G2V_ERR_WORKSPACE;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  if (F == 2 || smooth == 1.0) {                 // nothing to solve: the spline interpolates
    if (out != y) {
      if (hipMemcpyAsync(out, y, (size_t)B * F * Cn * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
        (void)hipGetLastError();
        set_error("g2v_smoothing_spline: the copy failed");
        return G2V_ERR_LAUNCH;
      }
    }
    return G2V_OK;
  }
  const int n = F - 2;
  const double q = 6.0 * (1.0 - smooth);
  double* fac = static_cast<double*>(workspace);
  double* w = fac + 3 * (size_t)n;
  const int64_t ncol = (int64_t)B * Cn;
  hipLaunchKernelGGL(spline_factor_kernel, dim3(1), dim3(64), 0, st, fac, n, 6.0 * q + 4.0 * smooth, -4.0 * q + smooth, q);
  G2V_CHECK_LAUNCH();
  hipLaunchKernelGGL(spline_sweep_kernel, dim3((unsigned)((ncol + 63) / 64)), dim3(64), 0, st, y, out, fac, w, F, Cn, ncol, q);
  G2V_CHECK_LAUNCH();
  return G2V_OK;
}

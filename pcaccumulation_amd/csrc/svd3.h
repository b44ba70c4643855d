// The 3x3 SVD behind every ego-motion pose (ego.hip: the fused eval kernel ego_kabsch_kernel and the differentiable svd3_kernel of the training
// path; toolbox/register_utils.py:296 `torch.svd(cov_mat)`), as ONE __host__ __device__ function, so that the SAME code runs in the kernels and
// in a g++ build (tests/svd3_host_driver.cpp) against LAPACK in float64 (only +, -, *, / and sqrt: the host factors rounded to float32 are the
// kernel's outputs bit for bit, tests/test_ego_solve.py::test_host_build_equals_the_kernel_bits).  Includes nothing of HIP.
//
// a = u diag(s) v^T by one-sided Jacobi rotations of the columns of a (a v = u diag(s)), float64, no FMA contraction, s descending and >= 0.
// Every decision is RELATIVE, so the factors of c * a are those of a for any c that keeps the squares inside float64 (s scales, u and v are
// bit-identical for c a power of two):
//   - a column pair (p, q) is left alone when |<b_p, b_q>| <= SVD3_PAIR_EPS * |b_p| |b_q|: the cosine of two columns of u.  A sweep that rotated
//     nothing ends the iteration (30 sweeps at most; quadratic convergence needs 4-6);
//   - a singular value at or below SVD3_RANK_TOL * s[0] counts as zero.  Its column of u is then not b_j / s[j] -- the direction of rounding
//     noise, or 0 / 0 -- but completes the columns that exist to a right-handed orthonormal basis: u_2 = u_0 x u_1 at rank 2; at rank 1
//     u_1 = the unit vector along u_0 x e_m (m the axis u_0 leans on least) and u_2 = u_0 x u_1; u = I at rank 0 (v = I there: nothing rotated).
// So u and v are orthonormal for every finite input, and v diag(1, 1, det(v u^T)) u^T is a proper rotation.  Where LAPACK's answer is a function
// of the matrix -- (s_1 + sign(det a) s_2) / s_0 away from 0 -- that rotation is LAPACK's; below, it is one valid choice inside the null space,
// the same one every run.  NaN goes in, NaN comes out.  The one 3x3 SVD of the library: the covariances of C5's normals (accum_normals.h) and
// of C3's ICP update (icp_round.h, through jacobi_svd3_floor) go through it as well.
#pragma once
#include <math.h>

#include "hd.h"

#define SVD3_PAIR_EPS 8.881784197001252e-16            // 4 * 2^-52: rounding leaves |cos| of two orthogonal columns at ~3 * 2^-53
#define SVD3_RANK_TOL 1.4210854715202004e-14           // 64 * 2^-52

// `zero_floor`: an absolute value at or below which a singular value counts as zero as well (0 = none) -- for a caller whose matrix carries rounding noise
// of a known size that is NOT relative to s[0] (icp_round.h: a covariance formed from uncentred sums).  Returns the rank, 0 .. 3.
PCACC_HD_PLAIN int jacobi_svd3_floor(const double a[3][3], double zero_floor, double u[3][3], double s[3], double v[3][3])
{
    PCACC_NO_CONTRACT
    double b[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { b[i][j] = a[i][j]; v[i][j] = (i == j); }
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int i = 0; i < 3; ++i) { alpha += b[i][p] * b[i][p]; beta += b[i][q] * b[i][q]; gamma += b[i][p] * b[i][q]; }
                if (fabs(gamma) <= SVD3_PAIR_EPS * sqrt(alpha * beta)) continue;             // orthogonal already (a zero column included)
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
                for (int i = 0; i < 3; ++i) {
                    const double bp = b[i][p], bq = b[i][q];
                    b[i][p] = c * bp - sn * bq; b[i][q] = sn * bp + c * bq;
                    const double vp = v[i][p], vq = v[i][q];
                    v[i][p] = c * vp - sn * vq; v[i][q] = sn * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    for (int j = 0; j < 3; ++j) {
        double n = 0;
        for (int i = 0; i < 3; ++i) n += b[i][j] * b[i][j];
        s[j] = sqrt(n);
    }
    // order singular values descending (as LAPACK / torch.svd)
    for (int x = 0; x < 2; ++x)
        for (int y = x + 1; y < 3; ++y)
            if (s[y] > s[x]) {
                const double ts = s[x]; s[x] = s[y]; s[y] = ts;
                for (int i = 0; i < 3; ++i) {
                    const double tb = b[i][x]; b[i][x] = b[i][y]; b[i][y] = tb;
                    const double tv = v[i][x]; v[i][x] = v[i][y]; v[i][y] = tv;
                }
            }
    if (s[0] <= zero_floor) {                                                                     // rank 0 (s[0] == 0 without a floor; NaN goes on)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) u[i][j] = (i == j);
        return 0;
    }
    double tol = SVD3_RANK_TOL * s[0];
    if (tol < zero_floor) tol = zero_floor;
    for (int i = 0; i < 3; ++i) u[i][0] = b[i][0] / s[0];
    if (s[1] > tol) {
        for (int i = 0; i < 3; ++i) u[i][1] = b[i][1] / s[1];
    } else {                                                                                 // rank 1: any unit vector orthogonal to u_0
        int m = 0;
        if (fabs(u[1][0]) < fabs(u[m][0])) m = 1;
        if (fabs(u[2][0]) < fabs(u[m][0])) m = 2;
        const double e[3] = {m == 0 ? 1.0 : 0.0, m == 1 ? 1.0 : 0.0, m == 2 ? 1.0 : 0.0};
        const double w[3] = {u[1][0] * e[2] - u[2][0] * e[1], u[2][0] * e[0] - u[0][0] * e[2], u[0][0] * e[1] - u[1][0] * e[0]};
        const double nw = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);                     // >= sqrt(2 / 3)
        for (int i = 0; i < 3; ++i) u[i][1] = w[i] / nw;
    }
    if (s[2] > tol) {                                                                        // s[1] >= s[2]: the second column exists as well
        for (int i = 0; i < 3; ++i) u[i][2] = b[i][2] / s[2];
    } else {                                                                                 // rank <= 2: complete U with a cross product
        u[0][2] = u[1][0] * u[2][1] - u[2][0] * u[1][1];
        u[1][2] = u[2][0] * u[0][1] - u[0][0] * u[2][1];
        u[2][2] = u[0][0] * u[1][1] - u[1][0] * u[0][1];
    }
    return 1 + (s[1] > tol) + (s[2] > tol);
}

PCACC_HD_PLAIN void jacobi_svd3(const double a[3][3], double u[3][3], double s[3], double v[3][3]) { (void)jacobi_svd3_floor(a, 0.0, u, s, v); }

// The scaffolding of every header whose arithmetic is a contract (svd3.h, icp_grid.h, icp_round.h, accum_grid.h, accum_normals.h, accum_register.h):
// such a header includes nothing of HIP, so that the SAME code runs in the kernels and in a g++ build (tests/*_host_driver.cpp, -ffp-contract=off
// -DPCACC_HOST_CHECK) where every table index is assert-checked before anything runs on a GPU.  One definition of each piece they share.
#pragma once
#include <stdint.h>

// PCACC_HD: host / device, force-inlined into the kernel.  PCACC_HD_PLAIN is plain `inline`: the decision is the compiler's (jacobi_svd3: large, several callers).
#if defined(__HIPCC__)
#define PCACC_HD __host__ __device__ __forceinline__
#define PCACC_HD_PLAIN __host__ __device__ inline
#else
#define PCACC_HD static inline
#define PCACC_HD_PLAIN static inline
#endif

// An index the code is about to use lies in [0, n): asserted in the host build, nothing in the kernels (their guards return -1 / skip instead).
// ACC_ / ICP_HOST_CHECK and ACC_ / ICP_BOUND alias this one definition: a host driver of the revision before this header builds against it, checks on.
#if defined(PCACC_HOST_CHECK) || defined(ACC_HOST_CHECK) || defined(ICP_HOST_CHECK)
#include <assert.h>
#define PCACC_BOUND(i, n) assert((int64_t)(i) >= 0 && (int64_t)(i) < (int64_t)(n))
#else
#define PCACC_BOUND(i, n) ((void)0)
#endif
#define ACC_BOUND PCACC_BOUND
#define ICP_BOUND PCACC_BOUND

// First statement of a function body: no FMA contraction in it, so that the kernels, the g++ build and a numpy restatement round alike.
#if defined(__clang__)
#define PCACC_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PCACC_NO_CONTRACT
#endif

#define PCACC_STOP_TOL 1e-6

PCACC_HD bool pcacc_finite(double v) { return v - v == 0.0; }           // false for NaN and +-Inf

// A fresh pose: rows 0-2 of init (NULL = identity), row 3 is 0 0 0 1.  T [16], row-major 4x4.
PCACC_HD void pcacc_pose_seed(double *T, const double *init)
{
    for (int k = 0; k < 12; ++k) T[k] = init ? init[k] : ((k % 5 == 0) ? 1.0 : 0.0);
    T[12] = T[13] = T[14] = 0.0;
    T[15] = 1.0;
}

// T <- [R | t] T on rows 0-2 of T: N_rc = ((R_r0 T_0c + R_r1 T_1c) + R_r2 T_2c), plus t_r for c = 3 only.  R [9] row-major.
PCACC_HD void pcacc_pose_compose(const double *R, const double *t, double *T)
{
    PCACC_NO_CONTRACT
    double N[12];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            const double v = (R[3 * r] * T[c] + R[3 * r + 1] * T[4 + c]) + R[3 * r + 2] * T[8 + c];
            N[4 * r + c] = c == 3 ? v + t[r] : v;
        }
    for (int k = 0; k < 12; ++k) T[k] = N[k];
}

// The stop rule of both ICP loops (Open3D's relative_fitness / relative_rmse at their defaults): an evaluation that moved neither figure.
PCACC_HD bool pcacc_icp_stop(double fit, double prev_fit, double rmse, double prev_rmse)
{
    PCACC_NO_CONTRACT
    return __builtin_fabs(fit - prev_fit) < PCACC_STOP_TOL && __builtin_fabs(rmse - prev_rmse) < PCACC_STOP_TOL;
}

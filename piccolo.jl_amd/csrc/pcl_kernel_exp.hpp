// pcl_kernel_exp.hpp -- the exact exponential integrator (pcl_desc.pade_order = PCL_ORDER_EXP): residual and Jacobian of
//     delta_k = X_{k+1} - exp(h G(u_k)) X_k ,   h = dt_k ,
// the reference's own constraint, for the step sizes no diagonal Pade order up to 10 follows.
//
//   d delta / d X_k     = -(I (x) E)            E = exp(h G)
//   d delta / d X_{k+1} = I                     (emitted as its diagonal)
//   d delta / d u_l     = -L_l X_k              L_l = the Frechet derivative of exp at h G along h G_l
//   d delta / d dt      = -G E X_k
//
//   pcl_exp_kernel<true>   one workgroup per (member, interval, drive l < max(m, 1)) -- 256 threads, 512 for n > 32 (sixteen output tiles per product: a
//                          pair per wave; the chain of products is the kernel's latency).  Each forms G(u_k) in LDS and runs the pair
//                          recurrence of pcl_var_expm_kernel with Gv = G_l -- the scaling theta = |h| |G|_1 <= 1/4, the Taylor degree 14 and the
//                          squaring count of pcl_expm_kernel; the T recurrence is that kernel's, expression for expression, so E has the
//                          rollout's bits:
//                              Horner    Tv <- f (G Tv + G_l T),  T <- I + f G T      (f = h 2^-s / j, j = 14 .. 1; Tv starts at 0)
//                              squaring  Tv <- T Tv + Tv T,       T <- T T
//                          then stores the l-th tail slice -L_l X_k of every state column.  E is recomputed by each of the m workgroups of an
//                          interval (one product in six per step): the workgroups stay independent -- no flag, no wait between them.  Every
//                          workgroup has E, so the cols copies of -E, the bulk of the bytes, are dealt round-robin over the interval's
//                          workgroups (16-byte stores); the one with l = 0 also stores delta, the dt tail and the ones of d/dX_{k+1}.
//                          m = 0: no Frechet pair, the T recurrence alone.
//   pcl_exp_kernel<false>  residual only: one workgroup per (member, interval), E alone -- the same T recurrence and the same product E X_k,
//                          hence the delta bits of the fused launch.
//   MODE (option exp_full; the default 0 is the kernel above, expression for expression -- every variant computes E, L_l and the products by
//   the same sequence, so delta and every value carry the bits of MODE 0):
//     PCL_EXP_COMPACT      the compact Jacobian: per interval [-E (n n) | tail], one copy of -E (stored by workgroup 0) and no ones
//                          (pcl_eval_jac_compact_dev; pcl_exp_expand_kernel replicates).
//     PCL_EXP_MERIT        the full values and, while the operands are in LDS, the reduce payload's partial sums (pcl_eval_jac_merit_dev):
//                          workgroup l leaves <lam, -L_l X_k> in part[bk (m + 2) + l], workgroup 0 also <lam, -G E X_k> in slot m and
//                          <lam, delta> in slot m + 1 (lam == NULL: lam = delta, slot m + 1 holds |delta|^2 / 2; a workgroup l > 0 then forms
//                          E X_k for itself, one more small product).  Each sum is reduced over the workgroup in a fixed order and written
//                          by a plain store: no atomic, no wait between workgroups; pcl_merit_sum_kernel finishes.
// Four rotating n x n tiles (G, T, Tv, one scratch; G's tile is the second scratch of the squarings) and the n x cols tile of X_k: 149 KB at
// n = 64 with 32 columns.  G_l has a fifth tile where that fits the LDS and is read from L2 by the product where not.  The products L_l X_k,
// E X_k and G (E X_k) land in spent tiles.  Every product goes through gemm_lds on the f64 matrix cores.
#pragma once

#define PCL_EXP_COMPACT 1
#define PCL_EXP_MERIT 2

template <bool JAC, int MODE = 0>
__global__ __launch_bounds__(512) void pcl_exp_kernel(const KParams p, const double *__restrict__ Gjd, const int gl_lds) {
    extern __shared__ double lds[];
    constexpr bool COMPACT = JAC && (MODE & PCL_EXP_COMPACT), MERIT = JAC && (MODE & PCL_EXP_MERIT);
    const int n = p.n, LD = p.LD, nn = n * n, cols = p.cols;
    const int tid = threadIdx.x, nth = blockDim.x;
    const int ml = JAC ? max(p.m, 1) : 1;
    const int l = blockIdx.x % ml;
    const long long bk = blockIdx.x / ml;
    const int k = (int)(bk % p.K), b = (int)(bk / p.K);
    const bool fre = JAC && p.m > 0;  // a Frechet pair is formed
    const int tile = LD * n;
    double *A = lds, *T = A + tile, *S = T + tile;
    double *X = JAC ? S + tile : nullptr;
    double *Gl = (fre && gl_lds) ? X + tile : nullptr;
    double *XK = lds + ((JAC ? 4 : 3) + (Gl ? 1 : 0)) * tile;
    double *us = XK + LD * cols, *red = us + 32;
    const double *zk = p.Z + (long long)b * p.z_batch_stride + (long long)k * p.z_dim;
    const double *G0 = p.G0 + (long long)b * p.g0_batch_stride;
    const double *Gv = fre ? Gjd + (long long)l * nn : nullptr;
    const double h = zk[p.dt_off];
    build_G(p, G0, zk, A, us);
    __syncthreads();
    if (tid < 64) {
        double cs = 0.0;
        if (tid < n)
            for (int i = 0; i < n; ++i) cs += fabs(A[i + LD * tid]);
        red[tid] = cs;
    }
    __syncthreads();
    double nrm = 0.0;
    for (int j = 0; j < n; ++j) nrm = fmax(nrm, red[j]);
    double theta = fabs(h) * nrm;
    int sq = 0;
    while (theta > 0.25 && sq < 60) {
        theta *= 0.5;
        ++sq;
    }
    const double hs = ldexp(h, -sq);
    for (int e = tid; e < nn; e += nth) {
        const int idx = (e % n) + LD * (e / n);
        T[idx] = (e % n == e / n) ? 1.0 : 0.0;
        if (fre) X[idx] = 0.0;
        if (Gl) Gl[idx] = Gv[e];
    }
    __syncthreads();
    for (int j = 14; j >= 1; --j) {
        const double f = hs / j;
        if (fre) {
            gemm_lds<true, false>(A, LD, X, LD, S, LD, n, n, n);  // S = G Tv
            __syncthreads();
            if (Gl)  // X = G_l T (the old Tv is spent)
                gemm_lds<true, false>(Gl, LD, T, LD, X, LD, n, n, n);
            else
                gemm_lds<true, false>(Gv, n, T, LD, X, LD, n, n, n);
            __syncthreads();
            for (int e = tid; e < nn; e += nth) {
                const int idx = (e % n) + LD * (e / n);
                S[idx] = f * (S[idx] + X[idx]);
            }
            double *t = X;  // Tv lives in S now
            X = S;
            S = t;
            __syncthreads();
        }
        gemm_lds<true, false>(A, LD, T, LD, S, LD, n, n, n);  // T <- I + f G T
        __syncthreads();
        for (int e = tid; e < nn; e += nth) {
            const int idx = (e % n) + LD * (e / n);
            T[idx] = ((e % n == e / n) ? 1.0 : 0.0) + f * S[idx];
        }
        __syncthreads();
    }
    for (int i = 0; i < sq; ++i) {
        if (fre) {
            gemm_lds<true, false>(T, LD, X, LD, S, LD, n, n, n);  // T Tv
            gemm_lds<true, false>(X, LD, T, LD, A, LD, n, n, n);  // Tv T (G is spent)
            __syncthreads();
            for (int e = tid; e < nn; e += nth) {
                const int idx = (e % n) + LD * (e / n);
                X[idx] = S[idx] + A[idx];
            }
            __syncthreads();
        }
        gemm_lds<true, false>(T, LD, T, LD, S, LD, n, n, n);
        __syncthreads();
        double *t = T;
        T = S;
        S = t;
    }
    // T = E, X = L_l; A (when a pair was squared) and S are free
    const int xo = p.x_off0 >= 0 ? p.x_off0 : p.x_offs[b];
    const int ne = n * cols;
    for (int e = tid; e < ne; e += nth) XK[(e % n) + LD * (e / n)] = zk[xo + e];
    __syncthreads();
    double *jv = JAC ? p.jac + bk * p.jac_per : nullptr;
    const int ncopy = COMPACT ? 1 : cols;  // copies of -E in the interval's block
    const long long seg1 = (long long)ncopy * nn, tail0 = seg1 + (COMPACT ? 0 : ne);
    const int tw = (p.m + 1) * n;  // tail doubles per state column
    const double *lam = MERIT && p.mlam ? p.mlam + bk * ne : nullptr;
    double *part = MERIT ? p.mpart + bk * (p.m + 2) : nullptr;
    if (fre) {
        gemm_lds<true, false>(X, LD, XK, LD, S, LD, n, cols, n);  // L_l X_k
        if (MERIT && !lam) gemm_lds<true, false>(T, LD, XK, LD, A, LD, n, cols, n);  // lam = delta: E X_k (G's tile; workgroup 0 builds G again)
        __syncthreads();
        for (int e = tid; e < ne; e += nth) jv[tail0 + (long long)(e / n) * tw + l * n + (e % n)] = -S[(e % n) + LD * (e / n)];
        if (MERIT) {
            double v = 0.0;
            for (int e = tid; e < ne; e += nth) {
                const int idx = (e % n) + LD * (e / n);
                v = fma(lam ? lam[e] : zk[p.z_dim + xo + e] - A[idx], -S[idx], v);
            }
            v = exph_block_sum(v, red);
            if (tid == 0) part[l] = v;
        }
        __syncthreads();
    }
    if (l == 0) {
        gemm_lds<true, false>(T, LD, XK, LD, S, LD, n, cols, n);  // E X_k
        __syncthreads();
        if (p.delta) {
            double *dl = p.delta + bk * ne;
            for (int e = tid; e < ne; e += nth) dl[e] = zk[p.z_dim + xo + e] - S[(e % n) + LD * (e / n)];
        }
        if (JAC) {
            if (fre && (sq > 0 || (MERIT && !lam))) {  // the squarings of the pair (or the payload's E X_k) went through G's tile
                build_G(p, G0, zk, A, us);
                __syncthreads();
            }
            gemm_lds<true, false>(A, LD, S, LD, X, LD, n, cols, n);  // G (E X_k); L_l is spent
            __syncthreads();
            for (int e = tid; e < ne; e += nth) {
                jv[tail0 + (long long)(e / n) * tw + p.m * n + (e % n)] = -X[(e % n) + LD * (e / n)];
                if (!COMPACT) jv[seg1 + e] = 1.0;
            }
            if (MERIT) {  // <lam, -G E X_k> and <lam, delta>; S = E X_k still
                double vh = 0.0, vp = 0.0;
                for (int e = tid; e < ne; e += nth) {
                    const int idx = (e % n) + LD * (e / n);
                    const double dl = zk[p.z_dim + xo + e] - S[idx], lm = lam ? lam[e] : dl;
                    vh = fma(lm, -X[idx], vh);
                    vp = fma(lm, dl, vp);
                }
                vh = exph_block_sum(vh, red);
                vp = exph_block_sum(vp, red);
                if (tid == 0) {
                    part[p.m] = vh;
                    part[p.m + 1] = lam ? vp : 0.5 * vp;
                }
            }
        }
    }
    if (JAC) {  // the copies of -E with c = l (mod ml)
        if (!(n & 1) && !((unsigned long long)jv & 15ull)) {
            const int half = nn >> 1;
            for (int c = l; c < ncopy; c += ml) {
                double *dst = jv + (long long)c * nn;
                for (int e2 = tid; e2 < half; e2 += nth) {
                    const int e = 2 * e2, idx = (e % n) + LD * (e / n);
                    const double2_t v = {-T[idx], -T[idx + 1]};
                    *reinterpret_cast<double2_t *>(dst + e) = v;
                }
            }
        } else {
            for (int c = l; c < ncopy; c += ml) {
                double *dst = jv + (long long)c * nn;
                for (int e = tid; e < nn; e += nth) dst[e] = -T[(e % n) + LD * (e / n)];
            }
        }
    }
}

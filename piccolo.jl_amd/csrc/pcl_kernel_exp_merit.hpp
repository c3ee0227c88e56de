// pcl_kernel_exp_merit.hpp -- the reduce payload of the exact exponential integrator without its Jacobian (PCL_ORDER_EXP with option
// exp_full = 1; pcl_eval_jac_merit_dev with vals == NULL):
//     g_u[k,l] = <Lam_k, d delta_k / d u_l> = -<Lam_k, L(A; h G_l) X_k>        g_dt[k] = <Lam_k, d delta_k / d dt> = -<Lam_k, G E X_k>
// with A = h G(u_k), E = exp(A), Lam_k the interval's multipliers reshaped like delta_k (NULL: delta_k itself).  The adjoint of the Frechet
// derivative, <W, L(A; P)> = <L(A'; W), P>, with W = Lam_k X_k' (n x n) and V = L(A'; W), gives every entry from ONE pair chain per interval:
//     <Lam, L(A; h G_l) X_k> = h <V, G_l>                  <Lam, G E X_k> = <W, L(A; G)> = <V, G> = <V, G0> + sum_l u_l <V, G_l>
// (G commutes with A, so L(A; G) = G E) -- where the Jacobian launch runs one chain per (interval, drive) and writes every value.
//
//   pcl_exp_hess_prep_kernel  (pcl_kernel_exp_hess.hpp, with Lam in the place of the multipliers M) leaves [G(u_k) | W | |G|_1] per interval in
//                             the context's workspace.
//   pcl_exp_merit_kernel      one workgroup per (member, interval) -- 256 threads, 512 for n > 32.  The pair recurrence of the Hessian kernel's
//                             (T, Tp) on A', with the Jacobian kernel's scaling (theta = |h| |G|_1 <= 1/4 after s halvings, Taylor degree 14,
//                             s squarings), a_h = h 2^-s / j, a_p = 2^-s / j:
//                                 Horner    V <- a_h G' V + a_p W T;   T <- I + a_h G' T            (j = 14 .. 1; V starts at 0)
//                                 squaring  V <- T V + V T;            T <- T T
//                             then the m + 1 inner products with G_l and G0 (read through L2) and <Lam, delta> (delta as the residual launch
//                             before it left it), each reduced over the workgroup in a fixed order and written by a plain store into the
//                             partial sums pcl_merit_sum_kernel finishes:  part[bk (m + 2) + l] = -h <V, G_l>,
//                             [.. + m] = -(<V, G0> + sum_l u_l <V, G_l>), [.. + m + 1] = <Lam, delta> (Lam = delta: half of it).
//                             No atomic, no wait between workgroups: two launches give the same bits.
// LDS: four n x n tiles (G(u_k), T, V, one scratch) and the reduction words: 135 296 B at n = 64.  W is read through L2 by the product.
#pragma once

__global__ __launch_bounds__(512) void pcl_exp_merit_kernel(const KParams p, const double *__restrict__ Gjd, const double *__restrict__ ws, const double *__restrict__ lam,
                                                            const double *__restrict__ delta, double *__restrict__ part) {
    extern __shared__ double lds[];
    const int n = p.n, LD = p.LD, nn = n * n, m = p.m;
    const int tid = threadIdx.x, nth = blockDim.x;
    const long long bk = blockIdx.x;
    const int k = (int)(bk % p.K), b = (int)(bk / p.K);
    const int tile = LD * n;
    double *Gt = lds, *T = Gt + tile, *V = T + tile, *S = V + tile, *red = S + tile;
    const double *zk = p.Z + (long long)b * p.z_batch_stride + (long long)k * p.z_dim;
    const double *Gg = ws + bk * (2LL * nn + 2), *Wg = Gg + nn;
    const double h = zk[p.dt_off];
    double theta = fabs(h) * Gg[2 * nn];
    int sq = 0;
    while (theta > 0.25 && sq < 60) {
        theta *= 0.5;
        ++sq;
    }
    const double hs = ldexp(h, -sq), ps = ldexp(1.0, -sq);
    for (int e = tid; e < nn; e += nth) {
        const int idx = (e % n) + LD * (e / n);
        T[idx] = (e % n == e / n) ? 1.0 : 0.0;
        V[idx] = 0.0;
        Gt[idx] = Gg[e];
    }
    __syncthreads();
    double *t_;
    for (int j = 14; j >= 1; --j) {
        const double ah = hs / j, ap = ps / j;
        gemm_lds_acc<true, false>(Gt, LD, V, LD, S, LD, n, n, n, ah);
        gemm_lds_acc<false, true>(Wg, n, T, LD, S, LD, n, n, n, ap);
        __syncthreads();
        t_ = S, S = V, V = t_;
        gemm_lds_acc<true, false>(Gt, LD, T, LD, S, LD, n, n, n, ah);
        __syncthreads();
        if (tid < n) S[tid + LD * tid] += 1.0;
        __syncthreads();
        t_ = S, S = T, T = t_;
    }
    for (int i = 0; i < sq; ++i) {
        gemm_lds_acc<false, false>(T, LD, V, LD, S, LD, n, n, n, 1.0);
        gemm_lds_acc<false, true>(V, LD, T, LD, S, LD, n, n, n, 1.0);
        __syncthreads();
        t_ = S, S = V, V = t_;
        gemm_lds_acc<false, false>(T, LD, T, LD, S, LD, n, n, n, 1.0);
        __syncthreads();
        t_ = S, S = T, T = t_;
    }
    // V = L(A'; W)
    double *out = part + bk * (m + 2);
    double gdt = 0.0;  // thread 0: sum_l u_l <V, G_l>, in drive order
    for (int l = 0; l < m; ++l) {
        const double *Gc = Gjd + (long long)l * nn;
        double v = 0.0;
        for (int e = tid; e < nn; e += nth) v = fma(V[(e % n) + LD * (e / n)], Gc[e], v);
        v = exph_block_sum(v, red);
        if (tid == 0) {
            out[l] = -h * v;
            gdt = fma(zk[p.u_off + l], v, gdt);
        }
    }
    const double *G0 = p.G0 + (long long)b * p.g0_batch_stride;
    double v0 = 0.0;
    for (int e = tid; e < nn; e += nth) v0 = fma(V[(e % n) + LD * (e / n)], G0[e], v0);
    v0 = exph_block_sum(v0, red);
    const long long ne = (long long)n * p.cols;
    const double *dl = delta + bk * ne, *lm = lam ? lam + bk * ne : dl;
    double vp = 0.0;
    for (long long e = tid; e < ne; e += nth) vp = fma(lm[e], dl[e], vp);
    vp = exph_block_sum(vp, red);
    if (tid == 0) {
        out[m] = -(v0 + gdt);
        out[m + 1] = lam ? vp : 0.5 * vp;
    }
}

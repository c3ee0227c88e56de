// pcl_kernel_exp_hess.hpp -- the Hessian of the Lagrangian of the exact exponential integrator (PCL_ORDER_EXP with option exp_hess = 1):
//     sum_k <M_k, delta_k>,   delta_k = X_{k+1} - exp(h G(u_k)) X_k ,   h = dt_k ,   M_k = the interval's multipliers reshaped like delta_k
// (DESIGN.md section 4.11).  Per interval the term is phi = -<W, exp(A)> with A = h G and W = M X_k' (n x n).  The adjoint of the Frechet
// derivative, <W, L(A; P)> = <L(A'; W), P>, turns the (u_i, u_j) block into one chain per drive instead of one per pair: with
//     T  = exp(A') = E'          Tp = L(A'; W)          Tq = L(A'; h G_l') = L_l'          Tw = L2(A'; W, h G_l')
//     (u_l, u_j)  = -h <Tw, G_j>            for every j (the row j <= l is stored)
//     (dt,  u_l)  = -<Tp, G_l> - <Tw, G>
//     (u_l, X_k)  = -Tq M
//     (dt,  X_k)  = -T (G' M)               (dt, dt) = -<G' T G' M, X_k>        (once per interval)
// Nothing involves X_{k+1}: the values per interval are  (u,u) lower triangle | (dt,u) | (dt,dt) | (u_l, X_k) l = 0 .. m-1 | (dt, X_k).
//
//   pcl_exp_hess_prep_kernel  one workgroup per (member, interval): G(u_k), its 1-norm (the squaring count) and W = M X_k' into the context's
//                             workspace, [G | W | norm] per interval -- the read-only left operands of the chain.
//   pcl_exp_hess_kernel       one workgroup per (member, interval, drive l < max(m, 1)) -- 256 threads, 512 for n > 32 -- independent of each other:
//                             no flag, no wait, no atomic.  The quadruple recurrence is the Jacobian kernel's pair recurrence one level up, with its
//                             scaling (theta = |h| |G|_1 <= 1/4 after s halvings, Taylor degree 14), a_h = h 2^-s / j, a_p = 2^-s / j:
//                                 Horner    Tw <- a_h G' Tw + a_p W Tq + a_h G_l' Tp;   Tp <- a_h G' Tp + a_p W T;
//                                           Tq <- a_h G' Tq + a_h G_l' T;              T  <- I + a_h G' T              (j = 14 .. 1)
//                                 squaring  Tw <- T Tw + Tw T + Tp Tq + Tq Tp;  Tp <- T Tp + Tp T;  Tq <- T Tq + Tq T;  T <- T T
//                             Every right-hand side reads the old tiles, so the sums land in the one scratch tile, which then trades places with
//                             the tile it replaces (mfma_gemm_lds_acc: the terms of a sum need no barrier between them).  Workgroup l owns row l
//                             of the (u,u) triangle, the (dt, u_l) entry and the (u_l, X_k) slice; workgroup 0 adds (dt,dt) and (dt, X_k); m = 0:
//                             the T recurrence alone.  Scalar entries are reduced inside the workgroup in a fixed order and written by plain
//                             stores: two launches give the same bits.
// LDS: five rotating n x n tiles (T, Tp, Tq, Tw, scratch); G(u_k) has a sixth where that fits (n <= 56) and is read from the workspace through
// L2 where not, as W and G_l always are.  M and the products of the last phase land in spent tiles.  Five tiles fit up to n = 62.
#pragma once

__global__ __launch_bounds__(256) void pcl_exp_hess_prep_kernel(const KParams p, double *__restrict__ ws) {
    extern __shared__ double lds[];
    const int n = p.n, LD = p.LD, nn = n * n, cols = p.cols;
    const int tid = threadIdx.x, nth = blockDim.x;
    const long long bk = blockIdx.x;
    const int k = (int)(bk % p.K), b = (int)(bk / p.K);
    double *A = lds, *us = A + LD * n, *red = us + 32;
    const double *zk = p.Z + (long long)b * p.z_batch_stride + (long long)k * p.z_dim;
    const double *G0 = p.G0 + (long long)b * p.g0_batch_stride;
    build_G(p, G0, zk, A, us);
    __syncthreads();
    if (tid < 64) {
        double cs = 0.0;
        if (tid < n)
            for (int i = 0; i < n; ++i) cs += fabs(A[i + LD * tid]);
        red[tid] = cs;
    }
    __syncthreads();
    const int xo = p.x_off0 >= 0 ? p.x_off0 : p.x_offs[b];
    const double *x = zk + xo, *mu = p.mu + bk * (long long)n * cols;
    double *xs = red + 64, *ms = xs + n * cols;  // X_k and M staged: every entry is read n times
    for (int e = tid; e < n * cols; e += nth) {
        xs[e] = x[e];
        ms[e] = mu[e];
    }
    __syncthreads();
    double *w = ws + bk * (2LL * nn + 2);
    for (int e = tid; e < nn; e += nth) {
        const int i = e % n, j = e / n;
        double s = 0.0;
        for (int c = 0; c < cols; ++c) s = fma(ms[i + n * c], xs[j + n * c], s);
        w[e] = A[i + LD * j];
        w[nn + e] = s;
    }
    if (tid == 0) {
        double nrm = 0.0;
        for (int j = 0; j < n; ++j) nrm = fmax(nrm, red[j]);
        w[2 * nn] = nrm;
    }
}

// sum over the workgroup of v, in a fixed order; the result is valid in thread 0 only.  red: one double per wave.
__device__ __forceinline__ double exph_block_sum(double v, double *red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
    __syncthreads();
    return s;
}

// C (+)= alpha G' B with G in its LDS tile or, where that tile does not fit, in the workspace
template <bool ACC>
__device__ __forceinline__ void exph_gt(const double *Gt, const double *Gg, const double *B, double *C, int LD, int n, int nc, double alpha) {
    if (Gt)
        gemm_lds_acc<true, ACC>(Gt, LD, B, LD, C, LD, n, nc, n, alpha);
    else
        gemm_lds_acc<true, ACC>(Gg, n, B, LD, C, LD, n, nc, n, alpha);
}

#define EXPH_SWAP(a, b) \
    do {                \
        double *t_ = a; \
        a = b;          \
        b = t_;         \
    } while (0)

__global__ __launch_bounds__(512) void pcl_exp_hess_kernel(const KParams p, const double *__restrict__ Gjd, const double *__restrict__ ws, const int g_lds) {
    extern __shared__ double lds[];
    const int n = p.n, LD = p.LD, nn = n * n, cols = p.cols, m = p.m;
    const int tid = threadIdx.x, nth = blockDim.x;
    const int ml = max(m, 1);
    const int l = blockIdx.x % ml;
    const long long bk = blockIdx.x / ml;
    const int k = (int)(bk % p.K), b = (int)(bk / p.K);
    const bool fre = m > 0;  // the quadruple is formed
    const int tile = LD * n;
    double *T = lds, *Tp = T + tile, *Tq = Tp + tile, *Tw = Tq + tile, *S = Tw + tile;
    double *Gt = g_lds ? S + tile : nullptr;
    double *red = lds + (g_lds ? 6 : 5) * tile;
    const double *zk = p.Z + (long long)b * p.z_batch_stride + (long long)k * p.z_dim;
    const double *Gg = ws + bk * (2LL * nn + 2), *Wg = Gg + nn;
    const double *Gv = fre ? Gjd + (long long)l * nn : nullptr;
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
        if (fre) Tp[idx] = Tq[idx] = Tw[idx] = 0.0;
        if (Gt) Gt[idx] = Gg[e];
    }
    __syncthreads();
    for (int j = 14; j >= 1; --j) {
        const double ah = hs / j, ap = ps / j;
        if (fre) {
            exph_gt<false>(Gt, Gg, Tw, S, LD, n, n, ah);
            gemm_lds_acc<false, true>(Wg, n, Tq, LD, S, LD, n, n, n, ap);
            gemm_lds_acc<true, true>(Gv, n, Tp, LD, S, LD, n, n, n, ah);
            __syncthreads();
            EXPH_SWAP(S, Tw);
            exph_gt<false>(Gt, Gg, Tp, S, LD, n, n, ah);
            gemm_lds_acc<false, true>(Wg, n, T, LD, S, LD, n, n, n, ap);
            __syncthreads();
            EXPH_SWAP(S, Tp);
            exph_gt<false>(Gt, Gg, Tq, S, LD, n, n, ah);
            gemm_lds_acc<true, true>(Gv, n, T, LD, S, LD, n, n, n, ah);
            __syncthreads();
            EXPH_SWAP(S, Tq);
        }
        exph_gt<false>(Gt, Gg, T, S, LD, n, n, ah);
        __syncthreads();
        if (tid < n) S[tid + LD * tid] += 1.0;
        __syncthreads();
        EXPH_SWAP(S, T);
    }
    for (int i = 0; i < sq; ++i) {
        if (fre) {
            gemm_lds_acc<false, false>(T, LD, Tw, LD, S, LD, n, n, n, 1.0);
            gemm_lds_acc<false, true>(Tw, LD, T, LD, S, LD, n, n, n, 1.0);
            gemm_lds_acc<false, true>(Tp, LD, Tq, LD, S, LD, n, n, n, 1.0);
            gemm_lds_acc<false, true>(Tq, LD, Tp, LD, S, LD, n, n, n, 1.0);
            __syncthreads();
            EXPH_SWAP(S, Tw);
            gemm_lds_acc<false, false>(T, LD, Tp, LD, S, LD, n, n, n, 1.0);
            gemm_lds_acc<false, true>(Tp, LD, T, LD, S, LD, n, n, n, 1.0);
            __syncthreads();
            EXPH_SWAP(S, Tp);
            gemm_lds_acc<false, false>(T, LD, Tq, LD, S, LD, n, n, n, 1.0);
            gemm_lds_acc<false, true>(Tq, LD, T, LD, S, LD, n, n, n, 1.0);
            __syncthreads();
            EXPH_SWAP(S, Tq);
        }
        gemm_lds_acc<false, false>(T, LD, T, LD, S, LD, n, n, n, 1.0);
        __syncthreads();
        EXPH_SWAP(S, T);
    }
    // T = E', Tp = L(A'; W), Tq = L_l', Tw = L2(A'; W, h G_l')
    double *hv = p.hess + bk * p.hess_per;
    const int nsc = (m + 1) * (m + 2) / 2, ne = n * cols;
    const double *mu = p.mu + bk * (long long)ne;
    if (fre) {
        for (int j = 0; j <= l; ++j) {  // row l of the (u,u) triangle
            const double *Gc = Gjd + (long long)j * nn;
            double v = 0.0;
            for (int e = tid; e < nn; e += nth) v = fma(Tw[(e % n) + LD * (e / n)], Gc[e], v);
            v = exph_block_sum(v, red);
            if (tid == 0) hv[l * (l + 1) / 2 + j] = -h * v;
        }
        double v1 = 0.0, v2 = 0.0;
        for (int e = tid; e < nn; e += nth) {
            const int idx = (e % n) + LD * (e / n);
            v1 = fma(Tp[idx], Gv[e], v1);
            v2 = fma(Tw[idx], Gg[e], v2);
        }
        v1 = exph_block_sum(v1, red);
        v2 = exph_block_sum(v2, red);
        if (tid == 0) hv[m * (m + 1) / 2 + l] = -v1 - v2;
    }
    double *XM = Tw, *U = Tp;  // both spent
    for (int e = tid; e < ne; e += nth) XM[(e % n) + LD * (e / n)] = mu[e];
    __syncthreads();
    if (fre) {
        gemm_lds_acc<false, false>(Tq, LD, XM, LD, S, LD, n, cols, n, 1.0);  // L_l' M
        __syncthreads();
        for (int e = tid; e < ne; e += nth) hv[nsc + (long long)l * ne + e] = -S[(e % n) + LD * (e / n)];
    }
    if (l == 0) {
        exph_gt<false>(Gt, Gg, XM, U, LD, n, cols, 1.0);  // G' M
        __syncthreads();
        gemm_lds_acc<false, false>(T, LD, U, LD, S, LD, n, cols, n, 1.0);  // E' G' M
        __syncthreads();
        for (int e = tid; e < ne; e += nth) hv[nsc + (long long)m * ne + e] = -S[(e % n) + LD * (e / n)];
        exph_gt<false>(Gt, Gg, S, U, LD, n, cols, 1.0);  // G' E' G' M
        __syncthreads();
        const int xo = p.x_off0 >= 0 ? p.x_off0 : p.x_offs[b];
        double v = 0.0;
        for (int e = tid; e < ne; e += nth) v = fma(U[(e % n) + LD * (e / n)], zk[xo + e], v);
        v = exph_block_sum(v, red);
        if (tid == 0) hv[nsc - 1] = -v;
    }
}
#undef EXPH_SWAP

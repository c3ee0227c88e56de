// pcl_kernel_var_rollout.hpp -- rollout of a variational context (option var_full): exact piecewise-constant propagation of the stacked state
// [X; Xv_1; ..; Xv_v] under the lifted generator var_G(G(u_k), [Gv_i]), without ever forming the (1 + v) n square lifted matrix.
//
// exp(h var_G(G, [Gv_i])) is block lower triangular: E = exp(h G) on the diagonal and, in block (i, 0), L_i = the Frechet derivative of exp at
// h G along h Gv_i.  So a knot costs  X <- E X,  Xv_i <- E Xv_i + L_i X.
//
//   pcl_var_expm_kernel   one workgroup per (interval, variation): the pair (E, L_i) with the scaling, the Taylor degree 14 and the squaring
//                         count of pcl_expm_kernel (theta = |h| |G|_1; the T recurrence is that kernel's, expression for expression, so E has
//                         its bits).  Differentiating the recurrences term by term:
//                             Horner    Tv <- f (G Tv + Gv T),  T <- I + f G T       (f = h 2^-s / j, j = 14 .. 1; Tv starts at 0)
//                             squaring  Tv <- T Tv + Tv T,      T <- T T
//                         Four n x n tiles rotate (G, T, Tv, one scratch; G's tile is the second scratch of the squarings): 135 KB at n = 64.
//                         Gv_i is constant: it has a fifth tile where that fits the LDS (d <= 30) and is read from L2 by the product where not.
//                         A workgroup per variation repeats T for v = 2 (6 products per step instead of 5) and keeps one LDS plan for every v.
//   pcl_var_chain_kernel  one workgroup per (variation, group of state columns): the K dependent steps.  The columns of X are independent, so
//                         groups of 16 run side by side; the workgroups of variation 1 write component 0.  E and L_i of the next step are
//                         loaded into registers while the three products of this step run (256 threads, launched so by the host).
// Every product goes through gemm_lds on the matrix cores; an output element's sum does not depend on how the columns are grouped.
#pragma once

#define PCL_VAR_ROLL_PF 16  // doubles of an n x n tile per thread of a 256-thread workgroup (n <= 64)

struct VarRollParams {
    const double *Z;
    double *xout;  // [N][(1 + v) n cols]
    double *expm;  // [K][1 + v][n n]: E, L_1 .. L_v
    const double *G0, *Gj, *Gv;
    int n, LD, cols, m, K, v, z_dim, u_off, dt_off;
    int cc;      // state columns per chain workgroup
    int gv_lds;  // Gv_i has a tile of its own
    int xo[PCL_VAR_MAXV + 1];
};

__global__ __launch_bounds__(256) void pcl_var_expm_kernel(const VarRollParams p) {
    extern __shared__ double lds[];
    const int n = p.n, LD = p.LD, nn = n * n;
    const int tid = threadIdx.x, nth = blockDim.x;
    const int k = blockIdx.x / p.v, iv = blockIdx.x % p.v;
    const int tile = LD * n;
    double *A = lds, *T = A + tile, *X = T + tile, *S = X + tile;
    double *Gl = p.gv_lds ? S + tile : nullptr;
    double *us = lds + (p.gv_lds ? 5 : 4) * tile, *red = us + 32;
    const double *zk = p.Z + (long long)k * p.z_dim;
    const double *Gv = p.Gv + (long long)iv * nn;
    const double h = zk[p.dt_off];
    if (tid < p.m) us[tid] = zk[p.u_off + tid];
    __syncthreads();
    for (int e = tid; e < nn; e += nth) {  // G(u_k) = G0 + sum_l u_l G_l, in drive order
        double g = p.G0[e];
        for (int l = 0; l < p.m; ++l) g += us[l] * p.Gj[(long long)l * nn + e];
        const int idx = (e % n) + LD * (e / n);
        A[idx] = g;
        T[idx] = (e % n == e / n) ? 1.0 : 0.0;
        X[idx] = 0.0;
        if (Gl) Gl[idx] = Gv[e];
    }
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
    for (int j = 14; j >= 1; --j) {
        const double f = hs / j;
        gemm_lds<true, false>(A, LD, X, LD, S, LD, n, n, n);  // S = G Tv
        __syncthreads();
        if (Gl)  // X = Gv T (the old Tv is spent)
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
        gemm_lds<true, false>(A, LD, T, LD, S, LD, n, n, n);  // T <- I + f G T
        __syncthreads();
        for (int e = tid; e < nn; e += nth) {
            const int idx = (e % n) + LD * (e / n);
            T[idx] = ((e % n == e / n) ? 1.0 : 0.0) + f * S[idx];
        }
        __syncthreads();
    }
    for (int i = 0; i < sq; ++i) {
        gemm_lds<true, false>(T, LD, X, LD, S, LD, n, n, n);  // T Tv
        gemm_lds<true, false>(X, LD, T, LD, A, LD, n, n, n);  // Tv T (G is spent)
        __syncthreads();
        for (int e = tid; e < nn; e += nth) {
            const int idx = (e % n) + LD * (e / n);
            X[idx] = S[idx] + A[idx];
        }
        __syncthreads();
        gemm_lds<true, false>(T, LD, T, LD, S, LD, n, n, n);
        __syncthreads();
        double *t = T;
        T = S;
        S = t;
    }
    double *E = p.expm + (long long)k * (1 + p.v) * nn, *Lo = E + (long long)(1 + iv) * nn;
    for (int e = tid; e < nn; e += nth) {
        const int idx = (e % n) + LD * (e / n);
        if (iv == 0) E[e] = T[idx];
        Lo[e] = X[idx];
    }
}

__global__ __launch_bounds__(256) void pcl_var_chain_kernel(const VarRollParams p) {
    extern __shared__ double lds[];
    const int n = p.n, LD = p.LD, nn = n * n;
    const int tid = threadIdx.x, nth = blockDim.x;
    const int nch = (p.cols + p.cc - 1) / p.cc;
    const int iv = blockIdx.x / nch, c0 = (blockIdx.x % nch) * p.cc;
    const int nc = min(p.cc, p.cols - c0);
    const int ctile = LD * p.cc, ne = n * nc;
    const long long xdc = (long long)n * p.cols, xd = xdc * (1 + p.v);
    double *E = lds, *Lm = E + LD * n, *Xa = Lm + LD * n, *Xb = Xa + ctile, *Va = Xb + ctile, *Vb = Va + ctile, *P = Vb + ctile;
    double *o0 = p.xout + (long long)c0 * n, *oi = o0 + (long long)(1 + iv) * xdc;
    const bool first = iv == 0;
    for (int e = tid; e < ne; e += nth) {
        const int idx = (e % n) + LD * (e / n);
        const double x = p.Z[p.xo[0] + (long long)c0 * n + e], xv = p.Z[p.xo[1 + iv] + (long long)c0 * n + e];
        Xa[idx] = x;
        Va[idx] = xv;
        if (first) o0[e] = x;
        oi[e] = xv;
    }
    double *cur = Xa, *oth = Xb, *curv = Va, *othv = Vb;
    // The step's E and L_i travel through registers: the loads of step k + 1 are in flight while the products of step k run.
    double pe[PCL_VAR_ROLL_PF], pl[PCL_VAR_ROLL_PF];
    auto fetch = [&](int k) {
        const double *Ek = p.expm + (long long)k * (1 + p.v) * nn, *Lk = Ek + (long long)(1 + iv) * nn;
#pragma unroll
        for (int q = 0; q < PCL_VAR_ROLL_PF; ++q) {
            const int e = tid + 256 * q;
            if (e < nn) pe[q] = Ek[e], pl[q] = Lk[e];
        }
    };
    fetch(0);
    const int wave = tid >> 6, lane = tid & 63;
    for (int k = 0; k < p.K; ++k) {
        __syncthreads();  // the previous step is complete (E, L and the `oth` tiles are free)
#pragma unroll
        for (int q = 0; q < PCL_VAR_ROLL_PF; ++q) {
            const int e = tid + 256 * q;
            if (e < nn) {
                const int idx = (e % n) + LD * (e / n);
                E[idx] = pe[q];
                Lm[idx] = pl[q];
            }
        }
        __syncthreads();
        if (k + 1 < p.K) fetch(k + 1);
        // three independent products of at most four tile pairs each: the second starts at wave 2, so that all four waves have tiles
        mfma_gemm_lds<false>(E, LD, cur, LD, oth, LD, n, nc, n, wave, 4, lane);
        mfma_gemm_lds<false>(E, LD, curv, LD, othv, LD, n, nc, n, (wave + 2) & 3, 4, lane);
        mfma_gemm_lds<false>(Lm, LD, cur, LD, P, LD, n, nc, n, wave, 4, lane);
        __syncthreads();
        for (int e = tid; e < ne; e += nth) {
            const int idx = (e % n) + LD * (e / n);
            const double xv = othv[idx] + P[idx];
            othv[idx] = xv;
            oi[(long long)(k + 1) * xd + e] = xv;
            if (first) o0[(long long)(k + 1) * xd + e] = oth[idx];
        }
        double *t = cur;
        cur = oth;
        oth = t;
        t = curv;
        curv = othv;
        othv = t;
    }
}

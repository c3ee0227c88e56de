// pcl_kernel_var_exp_hess.hpp -- the Hessian of the Lagrangian of the variational integrators on the exact exponential constraint (batch_mode
// PCL_BATCH_VARIATIONAL_EXP with option var_exp_hess = 1):
//     sum_k <M_0, delta_0> + sum_i <M_i, delta_i>,   delta_0 = X_{k+1} - E X_k,   delta_i = Xv_{i,k+1} - L_i X_k - E Xv_{i,k}
// with h = dt_k, G = G(u_k), A = h G, E = exp(A), L_i = L(A; h Gv_i).  Only the subtracted parts carry curvature, and nothing involves knot k+1:
//     phi = -<W_0, E> - sum_i <W_i, L(A; h Gv_i)>,     W_0 = M_0 X' + sum_i M_i Xv_i',     W_i = M_i X'
// The first term is the plain exponential Hessian (pcl_kernel_exp_hess.hpp) on W_0: the quadruple T, Ta, Tc, Tac at A', one chain per drive l.
// The second, by <W, L3(A; P, Q, R)> = <L3(A'; W, Q', R'), P>, is an octuple chain per (variation i, drive l) with the directions
// a = W_i, b = h Gv_i', c = h G_l':
//     T = E'    Ta = L(A'; a)    Tb = L_i'    Tc = L_l'    Tab = L2(a, b)    Tac = L2(a, c)    Tbc = L2_il'    Tabc = L3(a, b, c)
//     (u_l, u_j)     = -h <Tac^0_l, G_j> - sum_i h <Tabc_il, G_j>                                     (^0: of the quadruple)
//     (dt, u_l)      = -<Ta^0, G_l> - <Tac^0_l, G> - sum_i [ <Tab_i, G_l> + <Tabc_il, G> + <Tac_il, Gv_i> ]
//     (u_l, X_k)     = -(Tc_l M_0 + sum_i Tbc_il M_i)               (u_l, Xv_i,k) = -Tc_l M_i
//     (dt, X_k)      = -(T N_0 + sum_i Tb_i N_i)                    (dt, Xv_i,k)  = -T N_i          N_0 = G' M_0 + sum_i Gv_i' M_i,  N_i = G' M_i
//     (dt, dt)       = -<T R_0 + sum_i Tb_i R_i, X_k> - sum_i <T R_i, Xv_i,k>                       R_0 = G' N_0 + sum_i Gv_i' N_i,  R_i = G' N_i
// (N and R are the lifted generator's transpose applied once and twice to the stacked multipliers.)  The values per interval are the first
// five segments of the Pade variational layout: (u,u) lower triangle | (dt,u) | (dt,dt) | (u_l, X'_k) l = 0 .. m-1 | (dt, X'_k), X' the
// stacked state, component-major.
//
//   pcl_var_exp_hess_prep_kernel    one workgroup per interval: G(u_k) in drive order, its 1-norm (the squaring count), W_0 and the W_i into
//                                   the context's workspace, [G | norm | W_0 | W_1 .. W_v] per interval.
//   pcl_var_exp_hess_kernel<false>  the quadruple on W_0: one workgroup per (interval, drive l < max(m, 1)), five rotating n x LD tiles.
//   pcl_var_exp_hess_kernel<true>   the octuple: one workgroup per (interval, variation i, drive l < max(m, 1)), nine rotating tiles (eight
//                                   and the scratch).  256 threads, 512 for n > 32; independent workgroups: no flag, no wait, no atomic.
//                                   The scaling of the sibling kernels (theta = |h| |G|_1 <= 1/4 after s halvings, Taylor degree 14),
//                                   a_h = h 2^-s / j, a_p = 2^-s / j.  Horner, j = 14 .. 1, the highest tile first, every sum into the
//                                   scratch tile, which then trades places with the tile it replaces:
//                                       T_S <- a_h G' T_S + sum_{x in S} D_x T_{S \ x}  (+ I for S empty),   D_a = a_p W, D_b = a_h Gv_i', D_c = a_h G_l'
//                                   squaring, s times, the same order, old tiles only:  T_S <- sum_{R subset of S} T_R T_{S \ R}
//                                   (8 products for Tabc, 4 per double, 2 per single, 1 for T).  m = 0: the pair (T, Tb), resp. T alone.
//   pcl_var_exp_hess_finish_kernel  the entries several workgroups contribute to -- the (u,u) row, (dt, u_l), (dt, dt) and the component-0
//                                   slices of (u_l, X_k) and (dt, X_k) -- are written as partials [interval][1 + v][scalars | slices] (slot 0
//                                   the quadruple, slot i variation i) and added here in slot order: no floating-point atomic, two launches
//                                   give the same bits.  Everything else is written once by the workgroup that owns it.
// LDS: G(u_k) has a tile of its own where that fits (the sixth resp. tenth) and is read from the workspace through L2 where not, as W, Gv_i and
// G_l always are.  After the recurrences the spent tiles hold the n x cols products of the last phase (two per tile: cols <= n / 2), and in the
// octuple kernel the spent Ta holds the reduction words, so nine tiles are all it needs: n = 44 (145 728 B) is the largest shape of 160 KiB.
#pragma once

struct VarExpHessParams {
    const double *Z, *mu;
    double *hess;
    const double *G0, *Gj, *Gv;
    double *ws;    // [K][wsper]: G(u_k) | its 1-norm (two words) | W_0 | W_1 .. W_v
    double *part;  // [K][1 + v][pper]: scalars | (u_l, X_k) l = 0 .. m-1 | (dt, X_k)   (component 0)
    long long hper, wsper, pper;
    int n, LD, cols, m, K, v, z_dim, u_off, dt_off;
    int g_lds;  // G(u_k) has a tile of its own
    int xo[PCL_VAR_MAXV + 1];
};

__global__ __launch_bounds__(256) void pcl_var_exp_hess_prep_kernel(const VarExpHessParams p) {
    extern __shared__ double lds[];
    const int n = p.n, nn = n * n, cols = p.cols, v = p.v, ne = n * cols;
    const int tid = threadIdx.x, nth = blockDim.x;
    const int k = blockIdx.x;
    double *A = lds, *us = A + nn, *red = us + 32, *xs = red + 64, *ms = xs + (1 + v) * ne;
    const double *zk = p.Z + (long long)k * p.z_dim;
    const double *mu = p.mu + (long long)k * ne * (1 + v);
    double *w = p.ws + (long long)k * p.wsper;
    if (tid < p.m) us[tid] = zk[p.u_off + tid];
    for (int b = 0; b <= v; ++b)
        for (int e = tid; e < ne; e += nth) {
            xs[b * ne + e] = zk[p.xo[b] + e];
            ms[b * ne + e] = mu[b * ne + e];
        }
    __syncthreads();
    for (int e = tid; e < nn; e += nth) {  // G(u_k) = G0 + sum_l u_l G_l, in drive order
        double g = p.G0[e];
        for (int l = 0; l < p.m; ++l) g += us[l] * p.Gj[(long long)l * nn + e];
        A[e] = g;
        w[e] = g;
    }
    __syncthreads();
    if (tid < 64) {
        double cs = 0.0;
        if (tid < n)
            for (int i = 0; i < n; ++i) cs += fabs(A[i + n * tid]);
        red[tid] = cs;
    }
    __syncthreads();
    if (tid == 0) {
        double nrm = 0.0;
        for (int j = 0; j < n; ++j) nrm = fmax(nrm, red[j]);
        w[nn] = nrm;
        w[nn + 1] = 0.0;
    }
    double *W = w + nn + 2;
    for (int e = tid; e < nn; e += nth) {
        const int i = e % n, j = e / n;
        double s0 = 0.0;
        for (int b = 0; b <= v; ++b) {  // W_0 = M_0 X' + sum_i M_i Xv_i', in component order
            double sb = 0.0;
            for (int c = 0; c < cols; ++c) {
                s0 = fma(ms[b * ne + i + n * c], xs[b * ne + j + n * c], s0);
                if (b > 0) sb = fma(ms[b * ne + i + n * c], xs[j + n * c], sb);
            }
            if (b > 0) W[(long long)b * nn + e] = sb;  // W_i = M_i X'
        }
        W[e] = s0;
    }
}

#define VEH_SWAP(a, b)  \
    do {                \
        double *t_ = a; \
        a = b;          \
        b = t_;         \
    } while (0)
// terms of a Horner sum into the scratch tile S (the first of a sum is VEH_G): a_h G' X | a_p W X | a_h Gv_i' X | a_h G_l' X
#define VEH_G(X) exph_gt<false>(Gt, Gg, X, S, LD, n, n, ah)
#define VEH_W(X) gemm_lds_acc<false, true>(Wg, n, X, LD, S, LD, n, n, n, ap)
#define VEH_V(X) gemm_lds_acc<true, true>(Gvi, n, X, LD, S, LD, n, n, n, ah)
#define VEH_L(X) gemm_lds_acc<true, true>(Gl, n, X, LD, S, LD, n, n, n, ah)
// terms of a squaring sum: the first, the others
#define VEH_P0(X, Y) gemm_lds_acc<false, false>(X, LD, Y, LD, S, LD, n, n, n, 1.0)
#define VEH_P(X, Y) gemm_lds_acc<false, true>(X, LD, Y, LD, S, LD, n, n, n, 1.0)
// N_b of the last phase: the piece that holds it (v <= 2)
#define VEH_N(b) ((b) == 0 ? p0 : (b) == 1 ? p1 : p2)
// the sum is complete: S trades places with the tile it replaces
#define VEH_END(X)       \
    do {                 \
        __syncthreads(); \
        VEH_SWAP(S, X);  \
    } while (0)

// OCT = false: the quadruple (T, Ta, Tc, Tac) on W_0, workgroups (interval, l).  OCT = true: the octuple on W_i, workgroups (interval, i, l).
template <bool OCT>
__global__ __launch_bounds__(512) void pcl_var_exp_hess_kernel(const VarExpHessParams p) {
    extern __shared__ double lds[];
    const int n = p.n, LD = p.LD, nn = n * n, cols = p.cols, m = p.m, v = p.v;
    const int tid = threadIdx.x, nth = blockDim.x;
    const int ml = max(m, 1);
    const int l = blockIdx.x % ml;
    const int iv = OCT ? (blockIdx.x / ml) % v : 0;  // variation i = iv + 1
    const int k = OCT ? blockIdx.x / (ml * v) : blockIdx.x / ml;
    const bool fre = m > 0;  // the chains along a drive are formed
    const int tile = LD * n;
    constexpr int NT = OCT ? 9 : 5;
    double *T = lds, *Ta = T + tile, *Tc = Ta + tile, *Tac = Tc + tile, *S = Tac + tile;
    double *Tb = S + tile, *Tab = Tb + tile, *Tbc = Tab + tile, *Tabc = Tbc + tile;  // (the octuple's; never touched by the quadruple)
    double *Gt = p.g_lds ? lds + NT * tile : nullptr;
    const double *zk = p.Z + (long long)k * p.z_dim;
    const double *Gg = p.ws + (long long)k * p.wsper;
    const double *Wg = Gg + nn + 2 + (OCT ? (long long)(1 + iv) * nn : 0);
    const double *Gvi = p.Gv + (long long)iv * nn;
    const double *Gl = fre ? p.Gj + (long long)l * nn : nullptr;
    const double h = zk[p.dt_off];
    double theta = fabs(h) * Gg[nn];
    int sq = 0;
    while (theta > 0.25 && sq < 60) {
        theta *= 0.5;
        ++sq;
    }
    const double hs = ldexp(h, -sq), ps = ldexp(1.0, -sq);
    for (int e = tid; e < nn; e += nth) {
        const int idx = (e % n) + LD * (e / n);
        T[idx] = (e % n == e / n) ? 1.0 : 0.0;
        if (fre) Ta[idx] = Tc[idx] = Tac[idx] = 0.0;
        if (OCT) {
            Tb[idx] = 0.0;
            if (fre) Tab[idx] = Tbc[idx] = Tabc[idx] = 0.0;
        }
        if (Gt) Gt[idx] = Gg[e];
    }
    __syncthreads();
    for (int j = 14; j >= 1; --j) {
        const double ah = hs / j, ap = ps / j;
        if (OCT && fre) {
            VEH_G(Tabc), VEH_W(Tbc), VEH_V(Tac), VEH_L(Tab);
            VEH_END(Tabc);
            VEH_G(Tab), VEH_W(Tb), VEH_V(Ta);
            VEH_END(Tab);
        }
        if (fre) {
            VEH_G(Tac), VEH_W(Tc), VEH_L(Ta);
            VEH_END(Tac);
        }
        if (OCT && fre) {
            VEH_G(Tbc), VEH_V(Tc), VEH_L(Tb);
            VEH_END(Tbc);
        }
        if (fre) {
            VEH_G(Ta), VEH_W(T);
            VEH_END(Ta);
        }
        if (OCT) {
            VEH_G(Tb), VEH_V(T);
            VEH_END(Tb);
        }
        if (fre) {
            VEH_G(Tc), VEH_L(T);
            VEH_END(Tc);
        }
        VEH_G(T);
        __syncthreads();
        if (tid < n) S[tid + LD * tid] += 1.0;
        VEH_END(T);
    }
    for (int i = 0; i < sq; ++i) {
        if (OCT && fre) {
            VEH_P0(T, Tabc), VEH_P(Tabc, T), VEH_P(Ta, Tbc), VEH_P(Tbc, Ta), VEH_P(Tb, Tac), VEH_P(Tac, Tb), VEH_P(Tc, Tab), VEH_P(Tab, Tc);
            VEH_END(Tabc);
            VEH_P0(T, Tab), VEH_P(Tab, T), VEH_P(Ta, Tb), VEH_P(Tb, Ta);
            VEH_END(Tab);
        }
        if (fre) {
            VEH_P0(T, Tac), VEH_P(Tac, T), VEH_P(Ta, Tc), VEH_P(Tc, Ta);
            VEH_END(Tac);
        }
        if (OCT && fre) {
            VEH_P0(T, Tbc), VEH_P(Tbc, T), VEH_P(Tb, Tc), VEH_P(Tc, Tb);
            VEH_END(Tbc);
        }
        if (fre) {
            VEH_P0(T, Ta), VEH_P(Ta, T);
            VEH_END(Ta);
        }
        if (OCT) {
            VEH_P0(T, Tb), VEH_P(Tb, T);
            VEH_END(Tb);
        }
        if (fre) {
            VEH_P0(T, Tc), VEH_P(Tc, T);
            VEH_END(Tc);
        }
        VEH_P0(T, T);
        VEH_END(T);
    }
    // the tiles are final.  Reduction words: the quadruple kernel's own behind its tiles, the octuple kernel's in the spent Ta
    double *red = OCT ? Ta : lds + (NT + (p.g_lds ? 1 : 0)) * tile;
    const int nsc = (m + 1) * (m + 2) / 2, ne = n * cols;
    const long long xd = (long long)ne * (1 + v);
    double *hv = p.hess + (long long)k * p.hper;
    double *pt = p.part + ((long long)k * (1 + v) + (OCT ? 1 + iv : 0)) * p.pper;
    const double *mu = p.mu + (long long)k * xd;
    if (fre) {
        const double *Hi = OCT ? Tabc : Tac, *Mid = OCT ? Tab : Ta;
        for (int j = 0; j <= l; ++j) {  // row l of the (u,u) triangle
            const double *Gc = p.Gj + (long long)j * nn;
            double s = 0.0;
            for (int e = tid; e < nn; e += nth) s = fma(Hi[(e % n) + LD * (e / n)], Gc[e], s);
            s = exph_block_sum(s, red);
            if (tid == 0) pt[l * (l + 1) / 2 + j] = -h * s;
        }
        double v1 = 0.0, v2 = 0.0, v3 = 0.0;
        for (int e = tid; e < nn; e += nth) {
            const int idx = (e % n) + LD * (e / n);
            v1 = fma(Mid[idx], Gl[e], v1);
            v2 = fma(Hi[idx], Gg[e], v2);
            if (OCT) v3 = fma(Tac[idx], Gvi[e], v3);
        }
        v1 = exph_block_sum(v1, red);
        v2 = exph_block_sum(v2, red);
        if (OCT) v3 = exph_block_sum(v3, red);
        if (tid == 0) pt[m * (m + 1) / 2 + l] = OCT ? -v1 - v2 - v3 : -v1 - v2;
    }
    // three spent tiles, two n x cols pieces each (2 cols <= n: checked by var_exp_hess_enable)
    const int pc = LD * cols;
    double *F2 = OCT ? Tabc : Ta;
    double *p0 = Tac, *p1 = Tac + pc, *p2 = S, *p3 = S + pc, *p4 = F2, *p5 = F2 + pc;
    if (!OCT) {
        if (fre)
            for (int b = 0; b <= v; ++b) {  // -Tc_l M_b: component 0 shares its entries with the octuples, the others are this workgroup's
                for (int e = tid; e < ne; e += nth) p3[(e % n) + LD * (e / n)] = mu[(long long)b * ne + e];
                __syncthreads();
                gemm_lds_acc<false, false>(Tc, LD, p3, LD, p5, LD, n, cols, n, -1.0);
                __syncthreads();
                double *dst = b == 0 ? pt + nsc + (long long)l * ne : hv + nsc + l * xd + (long long)b * ne;
                for (int e = tid; e < ne; e += nth) dst[e] = p5[(e % n) + LD * (e / n)];
            }
        if (l == 0) {
            for (int b = 0; b <= v; ++b) {  // N_0 = G' M_0 + sum_i Gv_i' M_i (p0), N_i = G' M_i
                __syncthreads();
                for (int e = tid; e < ne; e += nth) p3[(e % n) + LD * (e / n)] = mu[(long long)b * ne + e];
                __syncthreads();
                exph_gt<false>(Gt, Gg, p3, VEH_N(b), LD, n, cols, 1.0);
                if (b > 0) gemm_lds_acc<true, true>(p.Gv + (long long)(b - 1) * nn, n, p3, LD, p0, LD, n, cols, n, 1.0);
            }
            for (int b = 0; b <= v; ++b) {  // (dt, X'_k): -T N_b
                __syncthreads();
                gemm_lds_acc<false, false>(T, LD, VEH_N(b), LD, p5, LD, n, cols, n, -1.0);
                __syncthreads();
                double *dst = b == 0 ? pt + nsc + (long long)m * ne : hv + nsc + m * xd + (long long)b * ne;
                for (int e = tid; e < ne; e += nth) dst[e] = p5[(e % n) + LD * (e / n)];
            }
            double acc = 0.0;
            for (int b = 0; b <= v; ++b) {  // (dt, dt): <T R_b, X'_b>,  R_0 = G' N_0 + sum_i Gv_i' N_i,  R_i = G' N_i
                __syncthreads();
                exph_gt<false>(Gt, Gg, VEH_N(b), p4, LD, n, cols, 1.0);
                if (b == 0)
                    for (int i = 1; i <= v; ++i) gemm_lds_acc<true, true>(p.Gv + (long long)(i - 1) * nn, n, VEH_N(i), LD, p4, LD, n, cols, n, 1.0);
                __syncthreads();
                gemm_lds_acc<false, false>(T, LD, p4, LD, p5, LD, n, cols, n, 1.0);
                __syncthreads();
                for (int e = tid; e < ne; e += nth) acc = fma(p5[(e % n) + LD * (e / n)], zk[p.xo[b] + e], acc);
            }
            acc = exph_block_sum(acc, red);
            if (tid == 0) pt[nsc - 1] = -acc;
        }
    } else {
        for (int e = tid; e < ne; e += nth) p3[(e % n) + LD * (e / n)] = mu[(long long)(1 + iv) * ne + e];
        __syncthreads();
        if (fre) {  // -Tbc_il M_i
            gemm_lds_acc<false, false>(Tbc, LD, p3, LD, p5, LD, n, cols, n, -1.0);
            __syncthreads();
            for (int e = tid; e < ne; e += nth) pt[nsc + (long long)l * ne + e] = p5[(e % n) + LD * (e / n)];
        }
        if (l == 0) {
            exph_gt<false>(Gt, Gg, p3, p1, LD, n, cols, 1.0);  // N_i
            __syncthreads();
            gemm_lds_acc<false, false>(Tb, LD, p1, LD, p5, LD, n, cols, n, -1.0);  // -Tb_i N_i
            exph_gt<false>(Gt, Gg, p1, p4, LD, n, cols, 1.0);                       // R_i
            __syncthreads();
            for (int e = tid; e < ne; e += nth) pt[nsc + (long long)m * ne + e] = p5[(e % n) + LD * (e / n)];
            __syncthreads();
            gemm_lds_acc<false, false>(Tb, LD, p4, LD, p5, LD, n, cols, n, 1.0);  // Tb_i R_i
            __syncthreads();
            double acc = 0.0;
            for (int e = tid; e < ne; e += nth) acc = fma(p5[(e % n) + LD * (e / n)], zk[p.xo[0] + e], acc);
            acc = exph_block_sum(acc, red);
            if (tid == 0) pt[nsc - 1] = -acc;
        }
    }
}
#undef VEH_N
#undef VEH_SWAP
#undef VEH_G
#undef VEH_W
#undef VEH_V
#undef VEH_L
#undef VEH_P0
#undef VEH_P
#undef VEH_END

// The shared entries: the 1 + v partials of an interval added in slot order.
__global__ __launch_bounds__(256) void pcl_var_exp_hess_finish_kernel(const VarExpHessParams p) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)p.K * p.pper) return;
    const long long k = idx / p.pper, e = idx % p.pper;
    const int nsc = (p.m + 1) * (p.m + 2) / 2, ne = p.n * p.cols;
    const double *pt = p.part + k * (1 + p.v) * p.pper + e;
    double s = pt[0];
    for (int i = 1; i <= p.v; ++i) s += pt[i * p.pper];
    const long long q = e - nsc;
    const long long dst = e < nsc ? e : nsc + (q / ne) * (long long)ne * (1 + p.v) + q % ne;
    p.hess[k * p.hper + dst] = s;
}

// pcl_kernel_var_exp.hpp -- the variational integrators on the exact exponential constraint (batch_mode PCL_BATCH_VARIATIONAL_EXP with
// pade_order = PCL_ORDER_EXP): residual and Jacobian of the stack [X; Xv_1; ..; Xv_v] under exp(h var_G(G(u_k), [Gv_i])),
// whose blocks are E = exp(A) on the diagonal and L_i = L(A; h Gv_i) in block (i, 0), A = h G(u_k), h = dt_k -- the lifted matrix is never formed:
//     delta_0 = X_{k+1} - E X_k                        delta_i = Xv_{i,k+1} - L_i X_k - E Xv_{i,k}
//     d delta_0 / d u_l = -L_l X_k                     d delta_i / d u_l = -(L2_il X_k + L_l Xv_{i,k})           L_l = L(A; h G_l), L2_il = L2(A; h Gv_i, h G_l)
//     d delta_0 / d dt  = -G Y_0                       d delta_i / d dt  = -(Gv_i Y_0 + G Y_i)                   Y_0 = E X_k, Y_i = L_i X_k + E Xv_{i,k}
// (the last line is -((Gv_i E + G L_i) X_k + G E Xv_{i,k}) with the two products that delta needs anyway).
//
//   pcl_var_exp_prep_kernel   one workgroup per interval: G(u_k) and its 1-norm into the context's workspace, [G | norm] per interval -- every
//                             workgroup of an interval reads one norm, so all of them take the same squaring count.
//   pcl_var_exp_kernel<true>  one workgroup per (interval, variation i, drive l < max(m, 1)) -- 256 threads, 512 for n > 32 -- independent of each other:
//                             no flag, no wait, no atomic, so two launches give the same bits.  The quadruple recurrence of pcl_exp_hess_kernel,
//                             not transposed, with its scaling (theta = |h| |G|_1 <= 1/4 after s halvings, Taylor degree 14), a = h 2^-s / j:
//                                 Horner    Tw <- a (G Tw + Gv_i Tq + G_l Tp);  Tp <- a (G Tp + Gv_i T);  Tq <- a (G Tq + G_l T);  T <- I + a G T
//                                 squaring  Tw <- T Tw + Tw T + Tp Tq + Tq Tp;  Tp <- T Tp + Tp T;  Tq <- T Tq + Tq T;  T <- T T
//                             leaves T = E, Tp = L_i, Tq = L_l, Tw = L2_il.  Workgroup (i, l) stores slice l of component i's tails; the workgroups
//                             of the first variation also store component 0's slice l; workgroup (i, 0) adds delta_i, the dt tail and the ones of
//                             component i, workgroup (1, 0) those of component 0.  The copies of -E (every workgroup of the interval has E) and of
//                             -L_i (the workgroups of variation i) are dealt round-robin over the workgroups that hold the tile, 16-byte stores.
//                             m = 0: the pair (T, Tp) alone.  A compact launch (VarExpParams::compact) stores [-E | -L_1 .. -L_v | tails]:
//                             -E once, by workgroup (1, 0); -L_i once, by workgroup (i, 0); no ones; the tails right behind the tiles.
//   pcl_var_exp_kernel<false> residual only: one workgroup per (interval, variation), the pair alone -- the same T and Tp recurrences and the same
//                             products Y_0, Y_i, hence the delta bits of the fused launch.
// LDS: five rotating n x n tiles (T, Tp, Tq, Tw, scratch); G(u_k) has a sixth where that fits (n <= 56) and is read from the workspace through L2
// where not, as Gv_i and G_l always are.  In the last phase [X_k | Xv_i,k] (n x 2 cols, cols <= n / 2) takes the spent scratch tile, the u_l tails go
// from the accumulators straight to their place in the values (the product's output tile is the values array, leading dimension (m + 1) n), and
// Y_0, Y_i land in the then spent Tq, Tw.  Five tiles fit up to n = 62.
#pragma once

struct VarExpParams {
    const double *Z;
    double *delta;  // may be null
    double *vals;   // null: residual only
    const double *G0, *Gj, *Gv;
    double *ws;  // [K][n n + 2]: G(u_k), its 1-norm
    long long jper;
    int n, LD, cols, m, K, v, z_dim, u_off, dt_off;
    int g_lds;  // G(u_k) has a tile of its own
    int compact;  // option var_compact: the values are [-E | -L_1 .. -L_v | tails], every tile once and no ones
    int xo[PCL_VAR_MAXV + 1];
};

__global__ __launch_bounds__(256) void pcl_var_exp_prep_kernel(const VarExpParams p) {
    __shared__ double A[4 * PCL_MAX_D * PCL_MAX_D], us[32], red[64];
    const int n = p.n, nn = n * n;
    const int tid = threadIdx.x, nth = blockDim.x;
    const int k = blockIdx.x;
    const double *zk = p.Z + (long long)k * p.z_dim;
    double *w = p.ws + (long long)k * (nn + 2);
    if (tid < p.m) us[tid] = zk[p.u_off + tid];
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
    }
}

// C (+)= alpha G B with G in its LDS tile or, where that tile does not fit, in the workspace
template <bool ACC>
__device__ __forceinline__ void vexp_g(const double *Gt, const double *Gg, const double *B, double *C, int ldc, int LD, int n, int nc, double alpha) {
    if (Gt)
        gemm_lds_acc<false, ACC>(Gt, LD, B, LD, C, ldc, n, nc, n, alpha);
    else
        gemm_lds_acc<false, ACC>(Gg, n, B, LD, C, ldc, n, nc, n, alpha);
}

#define VEXP_SWAP(a, b) \
    do {                \
        double *t_ = a; \
        a = b;          \
        b = t_;         \
    } while (0)

// the negated n x n tile S (leading dimension LD) to dst, 16 bytes per store where n is even and dst is aligned
__device__ __forceinline__ void vexp_store_neg(double *dst, const double *S, int LD, int n) {
    const int nn = n * n, tid = threadIdx.x, nth = blockDim.x;
    if (!(n & 1) && !((unsigned long long)dst & 15ull)) {
        for (int e2 = tid; e2 < (nn >> 1); e2 += nth) {
            const int e = 2 * e2, idx = (e % n) + LD * (e / n);
            const double2_t v = {-S[idx], -S[idx + 1]};
            *reinterpret_cast<double2_t *>(dst + e) = v;
        }
    } else {
        for (int e = tid; e < nn; e += nth) dst[e] = -S[(e % n) + LD * (e / n)];
    }
}

template <bool JAC>
__global__ __launch_bounds__(512) void pcl_var_exp_kernel(const VarExpParams p) {
    extern __shared__ double lds[];
    const int n = p.n, LD = p.LD, nn = n * n, cols = p.cols, m = p.m, v = p.v;
    const int tid = threadIdx.x, nth = blockDim.x;
    const int ml = JAC ? max(m, 1) : 1;
    const int l = blockIdx.x % ml;
    const int iv = (blockIdx.x / ml) % v;  // variation i = iv + 1
    const int k = blockIdx.x / (ml * v);
    const bool fre = JAC && m > 0;  // the quadruple is formed
    const int tile = LD * n;
    double *T = lds, *Tp = T + tile, *Tq = Tp + tile, *Tw = Tq + tile, *S = Tw + tile;
    double *Gt = p.g_lds ? S + tile : nullptr;
    const double *zk = p.Z + (long long)k * p.z_dim;
    const double *Gg = p.ws + (long long)k * (nn + 2);
    const double *Gvi = p.Gv + (long long)iv * nn;
    const double *Gl = fre ? p.Gj + (long long)l * nn : nullptr;
    const double h = zk[p.dt_off];
    double theta = fabs(h) * Gg[nn];
    int sq = 0;
    while (theta > 0.25 && sq < 60) {
        theta *= 0.5;
        ++sq;
    }
    const double hs = ldexp(h, -sq);
    for (int e = tid; e < nn; e += nth) {
        const int idx = (e % n) + LD * (e / n);
        T[idx] = (e % n == e / n) ? 1.0 : 0.0;
        Tp[idx] = 0.0;
        if (fre) Tq[idx] = Tw[idx] = 0.0;
        if (Gt) Gt[idx] = Gg[e];
    }
    __syncthreads();
    for (int j = 14; j >= 1; --j) {
        const double a = hs / j;
        if (fre) {
            vexp_g<false>(Gt, Gg, Tw, S, LD, LD, n, n, a);
            gemm_lds_acc<false, true>(Gvi, n, Tq, LD, S, LD, n, n, n, a);
            gemm_lds_acc<false, true>(Gl, n, Tp, LD, S, LD, n, n, n, a);
            __syncthreads();
            VEXP_SWAP(S, Tw);
        }
        vexp_g<false>(Gt, Gg, Tp, S, LD, LD, n, n, a);
        gemm_lds_acc<false, true>(Gvi, n, T, LD, S, LD, n, n, n, a);
        __syncthreads();
        VEXP_SWAP(S, Tp);
        if (fre) {
            vexp_g<false>(Gt, Gg, Tq, S, LD, LD, n, n, a);
            gemm_lds_acc<false, true>(Gl, n, T, LD, S, LD, n, n, n, a);
            __syncthreads();
            VEXP_SWAP(S, Tq);
        }
        vexp_g<false>(Gt, Gg, T, S, LD, LD, n, n, a);
        __syncthreads();
        if (tid < n) S[tid + LD * tid] += 1.0;
        __syncthreads();
        VEXP_SWAP(S, T);
    }
    for (int i = 0; i < sq; ++i) {
        if (fre) {
            gemm_lds_acc<false, false>(T, LD, Tw, LD, S, LD, n, n, n, 1.0);
            gemm_lds_acc<false, true>(Tw, LD, T, LD, S, LD, n, n, n, 1.0);
            gemm_lds_acc<false, true>(Tp, LD, Tq, LD, S, LD, n, n, n, 1.0);
            gemm_lds_acc<false, true>(Tq, LD, Tp, LD, S, LD, n, n, n, 1.0);
            __syncthreads();
            VEXP_SWAP(S, Tw);
        }
        gemm_lds_acc<false, false>(T, LD, Tp, LD, S, LD, n, n, n, 1.0);
        gemm_lds_acc<false, true>(Tp, LD, T, LD, S, LD, n, n, n, 1.0);
        __syncthreads();
        VEXP_SWAP(S, Tp);
        if (fre) {
            gemm_lds_acc<false, false>(T, LD, Tq, LD, S, LD, n, n, n, 1.0);
            gemm_lds_acc<false, true>(Tq, LD, T, LD, S, LD, n, n, n, 1.0);
            __syncthreads();
            VEXP_SWAP(S, Tq);
        }
        gemm_lds_acc<false, false>(T, LD, T, LD, S, LD, n, n, n, 1.0);
        __syncthreads();
        VEXP_SWAP(S, T);
    }
    // T = E, Tp = L_i, Tq = L_l, Tw = L2_il; S is free: [X_k | Xv_i,k]
    const int ne = n * cols;
    const long long xdc = ne, xd = xdc * (1 + v);
    double *X = S, *Xv = S + LD * cols;
    for (int e = tid; e < ne; e += nth) {
        const int idx = (e % n) + LD * (e / n);
        X[idx] = zk[p.xo[0] + e];
        Xv[idx] = zk[p.xo[1 + iv] + e];
    }
    __syncthreads();
    double *jv = JAC ? p.vals + (long long)k * p.jper : nullptr;
    const long long seg1 = (1LL + 2 * v) * cols * nn, tail0 = p.compact ? (1LL + v) * nn : seg1 + xd;
    const int tw = (m + 1) * n;  // tail doubles per state column
    double *t0 = JAC ? jv + tail0 : nullptr, *ti = JAC ? t0 + (long long)(1 + iv) * cols * tw : nullptr;  // the tails of component 0 and of component i
    if (fre) {  // the accumulators go to the values: column c of the product is state column c's slice l
        gemm_lds_acc<false, false>(Tw, LD, X, LD, ti + l * n, tw, n, cols, n, -1.0);
        gemm_lds_acc<false, true>(Tq, LD, Xv, LD, ti + l * n, tw, n, cols, n, -1.0);
        if (iv == 0) gemm_lds_acc<false, false>(Tq, LD, X, LD, t0 + l * n, tw, n, cols, n, -1.0);
        __syncthreads();  // Tq and Tw are spent
    }
    if (l == 0) {
        double *Y0 = Tq, *Yi = Tw;
        gemm_lds_acc<false, false>(T, LD, X, LD, Y0, LD, n, cols, n, 1.0);
        gemm_lds_acc<false, false>(Tp, LD, X, LD, Yi, LD, n, cols, n, 1.0);
        gemm_lds_acc<false, true>(T, LD, Xv, LD, Yi, LD, n, cols, n, 1.0);
        __syncthreads();
        if (p.delta) {
            double *dl = p.delta + (long long)k * xd;
            const double *zn = zk + p.z_dim;
            for (int e = tid; e < ne; e += nth) {
                const int idx = (e % n) + LD * (e / n);
                if (iv == 0) dl[e] = zn[p.xo[0] + e] - Y0[idx];
                dl[(1 + iv) * xdc + e] = zn[p.xo[1 + iv] + e] - Yi[idx];
            }
        }
        if (JAC) {
            gemm_lds_acc<false, false>(Gvi, n, Y0, LD, ti + m * n, tw, n, cols, n, -1.0);
            vexp_g<true>(Gt, Gg, Yi, ti + m * n, tw, LD, n, cols, -1.0);
            if (iv == 0) vexp_g<false>(Gt, Gg, Y0, t0 + m * n, tw, LD, n, cols, -1.0);
            for (int e = tid; e < ne && !p.compact; e += nth) {  // the identity's diagonal (the expansion writes it for a compact launch)
                if (iv == 0) jv[seg1 + e] = 1.0;
                jv[seg1 + (1 + iv) * xdc + e] = 1.0;
            }
        }
    }
    if (JAC && p.compact) {
        if (l == 0) {
            if (iv == 0) vexp_store_neg(jv, T, LD, n);
            vexp_store_neg(jv + (1LL + iv) * nn, Tp, LD, n);
        }
    } else if (JAC) {
        // blocks: -E (component 0) | per variation: -E, -L_i -- cols copies each.  The 1 + v blocks of -E are dealt over all v ml workgroups of
        // the interval, the block of -L_i over the ml workgroups of variation i.
        const int w = iv * ml + l, W = v * ml;
        for (int q = w; q < (1 + v) * cols; q += W) {
            const int comp = q / cols, c = q % cols;
            const long long blk = comp == 0 ? 0 : (2LL * comp - 1) * cols;
            vexp_store_neg(jv + (blk + c) * nn, T, LD, n);
        }
        for (int c = l; c < cols; c += ml) vexp_store_neg(jv + ((2LL * iv + 2) * cols + c) * nn, Tp, LD, n);
    }
}
#undef VEXP_SWAP

// pcl_kernel_var_exp_hess_tiles.hpp -- the octuple chain of pcl_kernel_var_exp_hess.hpp with four of its tiles in a device workspace (option
// var_exp_hess_tiles on a PCL_BATCH_VARIATIONAL_EXP context): generator dimensions 46 .. 62, where nine n x LD tiles
// exceed the LDS of a CU.  Prep, quadruple and finish kernels are those of the sibling header, and so are the partial-slot layout
// [interval][1 + v][pper] and the workgroups (interval, variation i, drive l < max(m, 1)); 256 threads, 512 for n > 32.
//
// What changes is only where a tile lives.  Per Horner step T is read by four products and Ta, Tb, Tc by three each: these and the scratch S
// rotate in LDS as before (five tiles: 163 680 B at n = 62, the footprint of the plain exponential Hessian kernel at its largest shape; G(u_k)
// has a sixth where that fits and comes from the workspace where not).  Tab, Tac, Tbc (read twice) and Tabc (read once) have FIXED homes
//     tiles[workgroup][Tab | Tac | Tbc | Tabc],   n x n each, column-major with leading dimension n
// and are read back through L2 as the B (or, in a squaring, A) operand of gemm_lds_acc, as W, Gv_i, G_l already are.  A sum that replaces a
// spilled tile is formed in S like every other and then copied to the tile's home with 16-byte stores (VEHT_SPILL, in place of the pointer
// swap): S stays the scratch, no pointer ever alternates between LDS and global memory.
//
// Order: the recurrence, its scaling and the order of its terms are those of pcl_var_exp_hess_kernel<true>, term for term -- the highest tile
// first, so a tile is replaced only after every sum that reads its old value -- and every product is the same gemm_lds_acc call of the same
// shape (a leading dimension does not enter the arithmetic).  The values are therefore the same bits as the LDS plan's wherever both run.
//
// Visibility: a home is written and read by its own workgroup only.  There is no hand-off between workgroups, no flag, no wait, no atomic.
// A workgroup runs on one CU, whose waves share one L1 that serves their vector memory operations in order: a store goes through that L1 to
// L2, and a load that any wave of the workgroup issues after the barrier is behind it and is served by the same L1 or by L2, never by a stale
// copy elsewhere.  __syncthreads() -- the barrier with its workgroup-scope release and acquire fences -- between the copy of a tile and its
// reads by other waves is therefore the whole protocol, as it is for the LDS tiles; the barrier before the copy keeps it behind the last read
// of the tile's old value.  (All accesses of the homes are vector loads and stores with per-lane addresses: nothing goes through the scalar cache.)
//
// Last phase: the pieces of the LDS plan sat in Tac, S and Tabc.  Here T and Tc are spent (the octuple's last phase takes Tbc and Tb as left
// operands only), Ta holds the reduction words as before, so the pieces are  N_i in T,  M_i in S,  R_i and the products in Tc  (two n x cols
// pieces per tile: 2 cols <= n, v <= 2, checked by var_exp_hess_enable).  The inner products <Tabc, G_j>, <Tab, G_l>, <Tabc, G>, <Tac, Gv_i>
// read the homes in the element order of the LDS plan.
#pragma once

// S -> home: n x n, LDS leading dimension LD to global leading dimension n; two doubles per lane and store (n and LD are even, a home starts
// at a multiple of 4 n^2 doubles)
__device__ __forceinline__ void veht_spill(const double *S, int LD, double *home, int n) {
    const int tid = threadIdx.x, nth = blockDim.x;
    if (n & 1) {
        for (int e = tid; e < n * n; e += nth) home[e] = S[(e % n) + LD * (e / n)];
        return;
    }
    const int hn = n >> 1;
    for (int q = tid; q < hn * n; q += nth) {
        const int i = 2 * (q % hn), j = q / hn;
        const double *s = S + i + LD * j;
        *reinterpret_cast<double2 *>(home + i + n * j) = make_double2(s[0], s[1]);
    }
}
// C (+)= alpha G' B, B with leading dimension ldb (exph_gt fixes it to LD)
template <bool ACC>
__device__ __forceinline__ void veht_gt(const double *Gt, const double *Gg, const double *B, int ldb, double *C, int LD, int n, int nc, double alpha) {
    if (Gt)
        gemm_lds_acc<true, ACC>(Gt, LD, B, ldb, C, LD, n, nc, n, alpha);
    else
        gemm_lds_acc<true, ACC>(Gg, n, B, ldb, C, LD, n, nc, n, alpha);
}

// terms of a Horner sum into the scratch tile S (the first of a sum is VEHT_G); X with leading dimension ldx: LD in LDS, n in its home
#define VEHT_G(X, ldx) veht_gt<false>(Gt, Gg, X, ldx, S, LD, n, n, ah)
#define VEHT_W(X, ldx) gemm_lds_acc<false, true>(Wg, n, X, ldx, S, LD, n, n, n, ap)
#define VEHT_V(X, ldx) gemm_lds_acc<true, true>(Gvi, n, X, ldx, S, LD, n, n, n, ah)
#define VEHT_L(X, ldx) gemm_lds_acc<true, true>(Gl, n, X, ldx, S, LD, n, n, n, ah)
// terms of a squaring sum: the first, the others
#define VEHT_P0(X, ldx, Y, ldy) gemm_lds_acc<false, false>(X, ldx, Y, ldy, S, LD, n, n, n, 1.0)
#define VEHT_P(X, ldx, Y, ldy) gemm_lds_acc<false, true>(X, ldx, Y, ldy, S, LD, n, n, n, 1.0)
// the sum is complete.  A resident tile: S trades places with it.  A spilled tile: S is copied to its home and stays the scratch.
#define VEHT_END(X)      \
    do {                 \
        __syncthreads(); \
        double *t_ = S;  \
        S = X;           \
        X = t_;          \
    } while (0)
#define VEHT_SPILL(X)             \
    do {                          \
        __syncthreads();          \
        veht_spill(S, LD, X, n);  \
        __syncthreads();          \
    } while (0)

__global__ __launch_bounds__(512) void pcl_var_exp_hess_tiles_kernel(const VarExpHessParams p, double *tiles) {
    extern __shared__ double lds[];
    const int n = p.n, LD = p.LD, nn = n * n, cols = p.cols, m = p.m, v = p.v;
    const int tid = threadIdx.x, nth = blockDim.x;
    const int ml = max(m, 1);
    const int l = blockIdx.x % ml;
    const int iv = (blockIdx.x / ml) % v;  // variation i = iv + 1
    const int k = blockIdx.x / (ml * v);
    const bool fre = m > 0;  // the chains along a drive are formed
    const int tile = LD * n;
    double *T = lds, *Ta = T + tile, *Tb = Ta + tile, *Tc = Tb + tile, *S = Tc + tile;  // resident: these five rotate
    double *Gt = p.g_lds ? lds + 5 * tile : nullptr;
    double *const Tab = tiles + (long long)blockIdx.x * 4 * nn, *const Tac = Tab + nn, *const Tbc = Tac + nn, *const Tabc = Tbc + nn;  // the homes
    const double *zk = p.Z + (long long)k * p.z_dim;
    const double *Gg = p.ws + (long long)k * p.wsper;
    const double *Wg = Gg + nn + 2 + (long long)(1 + iv) * nn;
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
        Tb[idx] = 0.0;
        if (fre) {
            Ta[idx] = Tc[idx] = 0.0;
            Tab[e] = Tac[e] = Tbc[e] = Tabc[e] = 0.0;
        }
        if (Gt) Gt[idx] = Gg[e];
    }
    __syncthreads();
    for (int j = 14; j >= 1; --j) {
        const double ah = hs / j, ap = ps / j;
        if (fre) {
            VEHT_G(Tabc, n), VEHT_W(Tbc, n), VEHT_V(Tac, n), VEHT_L(Tab, n);
            VEHT_SPILL(Tabc);
            VEHT_G(Tab, n), VEHT_W(Tb, LD), VEHT_V(Ta, LD);
            VEHT_SPILL(Tab);
            VEHT_G(Tac, n), VEHT_W(Tc, LD), VEHT_L(Ta, LD);
            VEHT_SPILL(Tac);
            VEHT_G(Tbc, n), VEHT_V(Tc, LD), VEHT_L(Tb, LD);
            VEHT_SPILL(Tbc);
            VEHT_G(Ta, LD), VEHT_W(T, LD);
            VEHT_END(Ta);
        }
        VEHT_G(Tb, LD), VEHT_V(T, LD);
        VEHT_END(Tb);
        if (fre) {
            VEHT_G(Tc, LD), VEHT_L(T, LD);
            VEHT_END(Tc);
        }
        VEHT_G(T, LD);
        __syncthreads();
        if (tid < n) S[tid + LD * tid] += 1.0;
        VEHT_END(T);
    }
    for (int i = 0; i < sq; ++i) {
        if (fre) {
            VEHT_P0(T, LD, Tabc, n), VEHT_P(Tabc, n, T, LD), VEHT_P(Ta, LD, Tbc, n), VEHT_P(Tbc, n, Ta, LD);
            VEHT_P(Tb, LD, Tac, n), VEHT_P(Tac, n, Tb, LD), VEHT_P(Tc, LD, Tab, n), VEHT_P(Tab, n, Tc, LD);
            VEHT_SPILL(Tabc);
            VEHT_P0(T, LD, Tab, n), VEHT_P(Tab, n, T, LD), VEHT_P(Ta, LD, Tb, LD), VEHT_P(Tb, LD, Ta, LD);
            VEHT_SPILL(Tab);
            VEHT_P0(T, LD, Tac, n), VEHT_P(Tac, n, T, LD), VEHT_P(Ta, LD, Tc, LD), VEHT_P(Tc, LD, Ta, LD);
            VEHT_SPILL(Tac);
            VEHT_P0(T, LD, Tbc, n), VEHT_P(Tbc, n, T, LD), VEHT_P(Tb, LD, Tc, LD), VEHT_P(Tc, LD, Tb, LD);
            VEHT_SPILL(Tbc);
            VEHT_P0(T, LD, Ta, LD), VEHT_P(Ta, LD, T, LD);
            VEHT_END(Ta);
        }
        VEHT_P0(T, LD, Tb, LD), VEHT_P(Tb, LD, T, LD);
        VEHT_END(Tb);
        if (fre) {
            VEHT_P0(T, LD, Tc, LD), VEHT_P(Tc, LD, T, LD);
            VEHT_END(Tc);
        }
        VEHT_P0(T, LD, T, LD);
        VEHT_END(T);
    }
    // the tiles are final.  Reduction words in the spent Ta, as in the LDS plan
    double *red = Ta;
    const int nsc = (m + 1) * (m + 2) / 2, ne = n * cols;
    const long long xd = (long long)ne * (1 + v);
    double *pt = p.part + ((long long)k * (1 + v) + 1 + iv) * p.pper;
    const double *mu = p.mu + (long long)k * xd;
    if (fre) {
        for (int j = 0; j <= l; ++j) {  // row l of the (u,u) triangle
            const double *Gc = p.Gj + (long long)j * nn;
            double s = 0.0;
            for (int e = tid; e < nn; e += nth) s = fma(Tabc[e], Gc[e], s);
            s = exph_block_sum(s, red);
            if (tid == 0) pt[l * (l + 1) / 2 + j] = -h * s;
        }
        double v1 = 0.0, v2 = 0.0, v3 = 0.0;
        for (int e = tid; e < nn; e += nth) {
            v1 = fma(Tab[e], Gl[e], v1);
            v2 = fma(Tabc[e], Gg[e], v2);
            v3 = fma(Tac[e], Gvi[e], v3);
        }
        v1 = exph_block_sum(v1, red);
        v2 = exph_block_sum(v2, red);
        v3 = exph_block_sum(v3, red);
        if (tid == 0) pt[m * (m + 1) / 2 + l] = -v1 - v2 - v3;
    }
    // the spent T, S and Tc: n x cols pieces (2 cols <= n)
    const int pc = LD * cols;
    double *p1 = T + pc, *p3 = S + pc, *p4 = Tc, *p5 = Tc + pc;
    for (int e = tid; e < ne; e += nth) p3[(e % n) + LD * (e / n)] = mu[(long long)(1 + iv) * ne + e];
    __syncthreads();
    if (fre) {  // -Tbc_il M_i
        gemm_lds_acc<false, false>(Tbc, n, p3, LD, p5, LD, n, cols, n, -1.0);
        __syncthreads();
        for (int e = tid; e < ne; e += nth) pt[nsc + (long long)l * ne + e] = p5[(e % n) + LD * (e / n)];
    }
    if (l == 0) {
        veht_gt<false>(Gt, Gg, p3, LD, p1, LD, n, cols, 1.0);  // N_i
        __syncthreads();
        gemm_lds_acc<false, false>(Tb, LD, p1, LD, p5, LD, n, cols, n, -1.0);  // -Tb_i N_i
        veht_gt<false>(Gt, Gg, p1, LD, p4, LD, n, cols, 1.0);                   // R_i
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
#undef VEHT_G
#undef VEHT_W
#undef VEHT_V
#undef VEHT_L
#undef VEHT_P0
#undef VEHT_P
#undef VEHT_END
#undef VEHT_SPILL

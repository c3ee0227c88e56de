// Rollout of the stacked state on a large variational context (PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR, 66 <= n <= 128; option
// large_var_full): from the knot-0 state,  x <- E x,  x_i <- E x_i + L_i x  per knot, E = exp(h G(u_k)), L_i the Frechet derivative of exp at h G
// along h Gv_i; output [N][(1 + v) n cols] -- the contract of pcl_var_expm_kernel + pcl_var_chain_kernel (pcl_kernel_var_rollout.hpp).  Those hold
// four or five n x n tiles; here ONE fits, so this is the two-launch plan of pcl_kernel_large_rollout.hpp with its helpers (lr_fetch_a, LR_DEG, LR_THETA,
// LR_SMAX) and those of pcl_device_large.hpp, and the lifted (1 + v) n square matrix is never formed.
//
//   pcl_var_large_expm_kernel   one workgroup per (interval, role, panel of npc columns).  Role 0 is E: the operations of pcl_large_expm_kernel in
//       its order (the bits of a plain PCL_LARGE_N context on the same drift and drives).  Role i = 1 .. v carries V again, with the same
//       operations and not stored, and Vv beside it; per substep, Horner for j = LR_DEG .. 1 with f = h_s / j
//           Vv <- Yv + f (G Vv + Gv_i V)        (the V before this level's update)
//           V  <- Y  + f G V
//       then Y <- V, Yv <- Vv; start Y = I[:, panel], Yv = 0.  G Vv and G V are ONE pass of matrix-core column tiles over the 2 npc columns of the
//       pair, the wave's rows of G in registers; Gv_i V is the row-compressed Gv_i against the old column of V in LDS (pl_row_dot, the row's fixed
//       order).  s' = ceil(|h| |G|_1) comes from the tile of G alone, clamped at LR_SMAX: every role and panel of an interval takes the same
//       substeps.  h = 0: s' = 0, E = I and L_i = 0 exactly; a negative h is an ordinary step.
//       LDS (doubles): G | three pairs [V | Vv] of npc columns each (Y, and the two the levels alternate between) | slack | us.
//       The panels go to the workspace [interval][E | L_1 .. L_v], n x n column-major each.
//   pcl_var_large_chain_kernel  one workgroup per (variation i, slice of nc <= 16 state columns): per knot  X' = E X,  Xv' = (E Xv) + (L_i X),
//       three products through pl_tile, the two of Xv' added once, in that order (the lane stores E Xv to LDS and adds L_i X to its own entry);
//       variation 1's workgroups store component 0.  The operands go from
//       the workspace straight into registers ahead of the product that uses them, STAGGERED so that two sets are live, not four:
//       E_k [X | Xv] runs while L_k is in flight, L_k X while E_{k+1} is (247 VGPRs, no scratch; with four sets, or with lr_fetch_a's
//       per-element addresses, the kernel spills).  LDS: two pairs [X | Xv] of nc columns | slack.
//
// Truncation: the argument of pcl_kernel_large_rollout.hpp with the lifted generator [[G, 0], [Gv_i, G]] in place of G: the Horner recurrence above
// IS the degree-18 polynomial of the lifted matrix applied to [V; Vv] (block lower triangular, so its (2, 1) block is the derivative of the
// polynomial along Gv_i); the substeps bound |h_s G|_1 <= 1, and the remainder of the derivative's series is that of exp'.
// Every element of every output is formed by one fixed sequence of operations whatever the split (panels, slices): no atomics, no sum across
// workgroups, the same bits from either pointer path and from every launch.
#pragma once

struct VarLargeRollParams {
    const double *gv_val;  // the variation generators row-compressed, [v][n][gv_w] (row-major, zero padded, columns ascending)
    const int *gv_col;
    int gv_w, v;
    int xo[1 + PCL_VAR_MAXV];  // state offsets of the components in the knot
    int npc, P;                // propagators: columns per panel, panels per role
    int nc, S;                 // chain: state columns per slice (<= 16), slices per variation
};

// p: Z, G0, upos / ucoef / n_upos (build_G), n, m, K, z_dim, u_off, dt_off, LD, lds_doubles, expm (the workspace)
__global__ __launch_bounds__(PL_NT) void pcl_var_large_expm_kernel(const KParams p, const VarLargeRollParams w) {
    extern __shared__ double lds[];
    const int n = p.n, LD = p.LD, npc = w.npc, P = w.P, v = w.v;
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, rt = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const long long bid = blockIdx.x, item = bid / P;
    const int u = (int)(bid % P);
    const int role = (int)(item % (1 + v));
    const long long k = item / (1 + v);
    const double *zk = p.Z + k * p.z_dim;
    const double h = zk[p.dt_off];
    const int pc0 = u * npc, npce = max(0, min(npc, n - pc0));
    const int PW = 2 * LD * npc;  // one pair [V | Vv]
    double *G = lds, *B0 = G + LD * n, *B1 = B0 + PW, *B2 = B1 + PW;
    double *us = B2 + PW + PL_SLACK;
    for (int e = tid; e < p.lds_doubles; e += nth) lds[e] = 0.0;
    __syncthreads();
    build_G(p, p.G0, zk, G, us);
    __syncthreads();
    // |G|_1 as pcl_large_expm_kernel forms it: the column sums go through the last pair (n <= 2 LD npc doubles; finite, and overwritten or
    // never used as a nonzero operand)
    if (tid < n) {
        double cs = 0.0;
        for (int i = 0; i < n; ++i) cs += fabs(G[i + LD * tid]);
        B2[tid] = cs;
    }
    __syncthreads();
    double nrm = 0.0;
    for (int j = 0; j < n; ++j) nrm = fmax(nrm, B2[j]);
    const double x = fabs(h) * nrm;
    const int sp = x == 0.0 ? 0 : (x <= (double)LR_SMAX * LR_THETA ? (int)ceil(x / LR_THETA) : LR_SMAX);
    const double hs = sp > 0 ? h / sp : 0.0;
    double a[PL_KS];
    const unsigned kmask = pl_load_a<false>(G, LD, n, rt, li, lk, a);
    __syncthreads();  // (the norms have been read: the last pair is free)
    for (int e = tid; e < npce * n; e += nth) {
        const int c = e / n, i = e - c * n;
        B0[i + LD * c] = (i == pc0 + c) ? 1.0 : 0.0;  // (Yv, behind it, is zero)
    }
    __syncthreads();
    double *Y = B0, *f1 = B1, *f2 = B2;
    const int cxp = role ? 2 * npc : npc, ct_n = (cxp + 15) >> 4;
    const int gw = w.gv_w;
    const long long vrow = (long long)(role - 1) * n;
    for (int s = 0; s < sp; ++s) {
        double *V = Y, *D = f1, *O = f2;
        for (int j = LR_DEG; j >= 1; --j) {
            const double f = hs / j;
            for (int ct = 0; ct < ct_n; ++ct) {
                const int vc = ct * 16 + li;
                const bool isv = vc >= npc;  // a column of Vv
                const int c = isv ? vc - npc : vc;
                const bool on = vc < cxp && c < npce;
                const double4_t acc = pl_tile(a, (on ? V + LD * vc : G) + lk, kmask);
                if (on) {
                    const int r0 = rt * 16 + lk;
                    if (!isv) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int rr = r0 + 4 * r;
                            if (rr < n) D[rr + LD * vc] = __builtin_fma(f, acc[r], Y[rr + LD * vc]);
                        }
                    } else {
                        // (rows beyond n - 1 read the last row; the stores are predicated)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int rr = r0 + 4 * r;
                            const double t = acc[r] + pl_row_dot(w.gv_val, w.gv_col, (vrow + min(rr, n - 1)) * gw, gw, V + LD * c);
                            if (rr < n) D[rr + LD * vc] = __builtin_fma(f, t, Y[rr + LD * vc]);
                        }
                    }
                }
            }
            __syncthreads();  // level j is complete in D; nothing reads V any more
            if (V == Y) {
                V = D;
                D = O;
            } else {
                double *t_ = V;
                V = D;
                D = t_;
            }
        }
        f1 = D;
        f2 = Y;
        Y = V;
    }
    const long long nn = (long long)n * n;
    pl_store_cols(p.expm + (k * (1 + v) + role) * nn + (long long)pc0 * n, role ? Y + LD * npc : Y, n, LD, npce, tid, nth);
}

// lr_fetch_a on one base pointer per lane (its row, its first k) and one stride: the operand's 32 addresses are then immediates of one register pair
__device__ __forceinline__ void vlr_fetch_a(const double *__restrict__ Er, int step, bool row_ok, int n, int lk, double (&a)[PL_KS]) {
#pragma unroll
    for (int ks = 0; ks < PL_KS; ++ks) a[ks] = (row_ok && 4 * ks + lk < n) ? Er[(long long)ks * step] : 0.0;
}

// p: Z, n, cols, K, LD, lds_doubles, expm (the workspace), xout
__global__ __launch_bounds__(PL_NT) void pcl_var_large_chain_kernel(const KParams p, const VarLargeRollParams w) {
    extern __shared__ double lds[];
    const int n = p.n, LD = p.LD, nc = w.nc, S = w.S, v = w.v;
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, rt = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int iv = (int)(blockIdx.x / S), s = (int)(blockIdx.x % S);  // variation iv + 1
    const int c0 = s * nc, nce = max(0, min(nc, p.cols - c0));
    const long long xdc = (long long)n * p.cols, xd = xdc * (1 + v), nn = (long long)n * n, wk = (1 + v) * nn;
    const int PW = 2 * LD * nc;  // one pair [X | Xv]
    double *cur = lds, *oth = lds + PW;
    const bool row_ok = rt * 16 + li < n;
    const int step = 4 * n;
    const double *Ew = p.expm + (rt * 16 + li) + (long long)n * lk, *Lw = Ew + (1 + iv) * nn;  // this lane's row and first k of every operand
    double ae[PL_KS], al[PL_KS];
    vlr_fetch_a(Ew, step, row_ok, n, lk, ae);  // (in flight while the state is loaded)
    for (int e = tid; e < p.lds_doubles; e += nth) lds[e] = 0.0;
    __syncthreads();
    const double *x0 = p.Z + w.xo[0] + (long long)c0 * n, *xv0 = p.Z + w.xo[1 + iv] + (long long)c0 * n;
    double *out0 = p.xout + (long long)c0 * n, *outv = out0 + (1 + iv) * xdc;
    const bool first = iv == 0;  // variation 1's workgroups store component 0
    for (int e = tid; e < nce * n; e += nth) {
        const int idx = (e % n) + LD * (e / n);
        const double xa = x0[e], xv = xv0[e];
        cur[idx] = xa;
        cur[LD * nc + idx] = xv;
        if (first) out0[e] = xa;
        outv[e] = xv;
    }
    __syncthreads();
    const bool on = li < nce;
    const int r0 = rt * 16 + lk;
    for (int k = 0; k < p.K; ++k) {
        unsigned kme = 0;
#pragma unroll
        for (int ks = 0; ks < PL_KS; ++ks)
            if (__ballot(ae[ks] != 0.0)) kme |= 1u << ks;
        kme = __builtin_amdgcn_readfirstlane(kme);
        vlr_fetch_a(Lw + k * wk, step, row_ok, n, lk, al);  // L_k: in flight during the two products with E_k
        const double4_t ax = pl_tile(ae, cur + (on ? LD * li : 0) + lk, kme);
        const double4_t av = pl_tile(ae, cur + (on ? LD * (nc + li) : 0) + lk, kme);
        if (on) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = r0 + 4 * r;
                if (rr < n) {
                    oth[rr + LD * li] = ax[r];
                    oth[rr + LD * (nc + li)] = av[r];
                }
            }
        }
        if (k + 1 < p.K) vlr_fetch_a(Ew + (k + 1) * wk, step, row_ok, n, lk, ae);  // E_{k+1}: in flight during the product with L_k
        unsigned kml = 0;
#pragma unroll
        for (int ks = 0; ks < PL_KS; ++ks)
            if (__ballot(al[ks] != 0.0)) kml |= 1u << ks;
        kml = __builtin_amdgcn_readfirstlane(kml);
        const double4_t aw = pl_tile(al, cur + (on ? LD * li : 0) + lk, kml);
        if (on) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = r0 + 4 * r;
                if (rr < n) oth[rr + LD * (nc + li)] += aw[r];  // (E Xv) + (L X): this lane's own store above
            }
        }
        __syncthreads();  // knot k + 1 is complete in `oth`; nothing reads `cur` any more (the next products write it)
        if (first) pl_store_cols(out0 + (long long)(k + 1) * xd, oth, n, LD, nce, tid, nth);
        pl_store_cols(outv + (long long)(k + 1) * xd, oth + LD * nc, n, LD, nce, tid, nth);
        double *t_ = cur;
        cur = oth;
        oth = t_;
    }
}

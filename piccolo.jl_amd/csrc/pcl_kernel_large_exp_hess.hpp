// Hessian of the Lagrangian on a large exponential context (PCL_LARGE_N | PCL_LARGE_EXP, pade_order = PCL_ORDER_EXP, 66 <= n <= 128; option
// large_exp_hess): values, order and layout are those of pcl_exp_hess_kernel (pcl_kernel_exp_hess.hpp) for the same KParams -- per interval the
// (m + 1)(m + 2) / 2 scalars [(u_i,u_l), l <= i | (dt,u_l) | (dt,dt)], then the vectors [(u_l, X_k) | (dt, X_k)], nothing on X_{k+1}.
//
// With h = dt_k, G = G(u_k), E = exp(h G), X = X_k, M = the interval's multipliers (n x cols), L_l = L(hG; hG_l), L2 the second Frechet derivative:
//   (u_i,u_l) = -<M, L2(hG; hG_i, hG_l) X>     (dt,u_l) = -<M, (G_l E + G L_l) X>     (dt,dt) = -<M, G^2 E X>     (u_l,X_k) = -L_l^T M     (dt,X_k) = -(G E)^T M
// Everything is a quantity of the ADJOINT chain on G^T started from M: the machinery is that of pcl_kernel_large_exp.hpp (ONE n x n tile, LD = n | 1,
// one wave per 16-row tile with its MFMA A operand -- here G^T, the tile's columns -- in registers over the whole loop, three rotating buffers, zero-
// filled LDS and PL_SLACK, one barrier per level), transposed, with one more derivative level carried.  s' = ceil(|h| |G|_1) substeps of h_s = h / s'
// (the norm and the clamp of that kernel: the same bits, the same s').  Per substep, from Y (at first M), dY_l (at first 0) and d2Y_il (l <= i, at
// first 0), Horner for j = LE_DEG .. 1 with f = h_s / j, every right-hand side with the values from BEFORE this level's update:
//       d2W_il <- d2Y_il + f (G^T d2W_il + G_i^T dW_l + G_l^T dW_i)
//       dW_l   <- dY_l   + f (G^T dW_l   + G_l^T W)
//       W      <- Y      + f  G^T W
// then Y <- W, dY_l <- dW_l, d2Y_il <- d2W_il.  After the last substep W = E^T M, dW_l = L_l^T M, d2W_il = L2(.; hG_i, hG_l)^T-action on M, and
//       (u_i,u_l) = -sum_cols <d2W_il, X>     (dt,u_l) = -<dW_l, G X> - <W, G_l X>     (dt,dt) = -<G^T W, G X>     (u_l,X_k) = -dW_l     (dt,X_k) = -G^T W
// (E commutes with G: d_u (E G) = L_l G + E G_l; no forward chain on X, only the one product G X, formed with the A registers reloaded).  h = 0:
// s' = 0, the (u,u) and (u,X) entries are exact zeros.  The sparse terms G_l^T (.) come from the ELL rows of G_l^T in memory, G_l X from those of G_l.
//
// Units: one workgroup per (interval, slice s of nc state columns, pair of drive groups (I, J), J <= I, of at most mg drives each):
// u = s + sx pr, pr = I (I + 1) / 2 + J.  Per state column a unit carries W, the dW of I (and of J off the diagonal) and the d2W of I x J
// (l <= i on the diagonal): blocks of nc columns  W | dW_I (mg) | dW_J (mg, off the diagonal) | d2W.  Every unit forms W and its dW with the same
// operations, hence the same bits.  Unit (0,0) stores (dt,X_k) and the (dt,dt) partials, the diagonal units (u_l,X_k) and the (dt,u_l) partials of
// their drives, every unit the (u_i,u_l) partials of its pairs.  A pair's sparse term is the drive with the larger index first, whatever the unit.
// LDS (doubles): G | three buffers of Wc columns | slack | us;  Wc = nc (1 + 2 mg + mg^2), the off-diagonal count, wherever there is more than one
// group; one group: nc (1 + mg + mg (mg + 1) / 2); no drives: 2 nc (W alone, and [X_k | G X_k] behind the chain).
//
// Determinism: no atomics.  A column's partial sums are formed by one wave per (column, entry), lanes over the rows, one shuffle tree, into the
// workspace p.hpart: [interval][column][(m + 1)(m + 2) / 2]; every entry has exactly one writer.  pcl_large_exp_hess_sum_kernel (the same stream,
// behind this launch) adds the columns in column order.  Every split (sx, mg) gives the same bits, and so do two launches.
//
// Truncation (pcl_kernel_large_exp.hpp, one level up).  With A = h_s G, |A|_1 <= 1: |d2(A^j)| <= j (j - 1) |A|^(j-2) |dA_i| |dA_l|, so the second
// derivative of the degree-18 polynomial misses at most  sum_{j >= 19} 1 / (j - 2)! = sum_{j >= 17} 1 / j! < 3.0e-15  of |h_s G_i| |h_s G_l| per substep.
#pragma once

// p.nc state columns per slice, p.lds_doubles to zero-fill; sx slices, mg drives per group, ngrp groups, Wc columns per buffer
__global__ __launch_bounds__(PL_NT) void pcl_large_exp_hess_kernel(const KParams p, const int sx, const int mg, const int ngrp, const int Wc) {
    extern __shared__ double lds[];
    const int n = p.n, d = p.cols, m = p.m, LD = p.LD, nc = p.nc;
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, rt = tid >> 6, nw = nth >> 6;  // one wave per row tile
    const int li = lane & 15, lk = lane >> 4;
    const int npr = ngrp * (ngrp + 1) / 2, U = sx * npr;
    const long long bid = blockIdx.x;
    const long long item = bid / U;
    const int u = (int)(bid % U);
    const int k = (int)(item % p.K), b = (int)(item / p.K);
    const int s_ = u % sx, pr = u / sx;
    int gI = 0;
    while ((gI + 1) * (gI + 2) / 2 <= pr) ++gI;  // pr = gI (gI + 1) / 2 + gJ, gJ <= gI
    const int gJ = pr - gI * (gI + 1) / 2;
    const bool diag = gI == gJ;
    const int c0 = s_ * nc, nce = max(0, min(nc, d - c0));  // this unit's state columns
    const int lI = gI * mg, lJ = gJ * mg;                    // ... and drives
    const int mgeI = m > 0 ? max(0, min(mg, m - lI)) : 0, mgeJ = m > 0 ? max(0, min(mg, m - lJ)) : 0;
    const int ndb = m > 0 ? (diag ? mg : 2 * mg) : 0;        // dW blocks
    const int npb = m > 0 ? (diag ? mg * (mg + 1) / 2 : mg * mg) : 0;  // d2W blocks
    const int T = 1 + ndb + npb, cx = T * nc;
    const double *zk = p.Z + (long long)b * p.z_batch_stride + (long long)k * p.z_dim;
    const double h = zk[p.dt_off];
    const long long xd = (long long)n * d;
    const double *mu = p.mu + item * xd;
    double *G = lds, *B0 = G + LD * n, *B1 = B0 + LD * Wc, *B2 = B1 + LD * Wc;
    double *us = B2 + LD * Wc + PL_SLACK;
    for (int e = tid; e < p.lds_doubles; e += nth) lds[e] = 0.0;
    __syncthreads();
    const int x_off = p.x_offs[p.z_batch_stride ? 0 : b];
    build_G(p, p.G0 + (long long)b * p.g0_batch_stride, zk, G, us);
    __syncthreads();
    // |G|_1 and s': the routine of pcl_large_exp_kernel (the column sums go through the third buffer)
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
    // A = G^T (the tile's columns)
    double a[PL_KS];
    unsigned kmask = pl_load_a<true>(G, LD, n, rt, li, lk, a);
    __syncthreads();  // (the norms have been read)
    if (tid < n) B2[tid] = 0.0;
    for (int e = tid; e < nce * n; e += nth) {  // Y = M; the dY and d2Y blocks stay zero
        const int c = e / n, i = e - c * n;
        B0[i + LD * c] = mu[(long long)(c0 + c) * n + i];
    }
    __syncthreads();
    double *Y = B0, *f1 = B1, *f2 = B2;
    const int ct_n = (cx + 15) >> 4;
    const int etw = p.ellt_w, ew = p.ell_w;
    for (int st = 0; st < sp; ++st) {
        double *V = Y, *D = f1, *O = f2;
        for (int j = LE_DEG; j >= 1; --j) {
            const double f = hs / j;
            for (int ct = 0; ct < ct_n; ++ct) {
                const int vc = ct * 16 + li;
                const int bl = vc / nc, c = vc - bl * nc;
                // block bl: 0 W | 1 + t dW (t < mg: drive lI + t, else lJ + t - mg) | 1 + ndb + q d2W of the pair q = (ai, bj)
                int kind = 0, l1 = 0, l2 = 0, s1 = 0, s2 = 0;  // kind 1: + G_l1^T (block s1); kind 2: + G_l1^T (block s1) + G_l2^T (block s2)
                bool on = vc < cx && c < nce;
                if (on && bl >= 1 && bl <= ndb) {
                    const int t = bl - 1;
                    kind = 1, s1 = 0;
                    l1 = t < mg ? lI + t : lJ + t - mg;
                    on = on && (t < mg ? t < mgeI : t - mg < mgeJ);
                } else if (on && bl > ndb) {
                    const int q = bl - 1 - ndb;
                    int ai, bj;
                    if (diag) {
                        ai = 0;
                        while ((ai + 1) * (ai + 2) / 2 <= q) ++ai;
                        bj = q - ai * (ai + 1) / 2;
                    } else {
                        ai = q / mg;
                        bj = q - ai * mg;
                    }
                    kind = 2;
                    l1 = lI + ai, s1 = diag ? 1 + bj : 1 + mg + bj;  // G_i^T dW_l: i = lI + ai >= l = lJ + bj
                    l2 = lJ + bj, s2 = 1 + ai;                       // G_l^T dW_i
                    on = on && ai < mgeI && bj < mgeJ;
                }
                const double4_t acc = pl_tile(a, (on ? V + LD * vc : G) + lk, kmask);
                if (on) {
                    const int r0 = rt * 16 + lk;
                    double y[4] = {0.0, 0.0, 0.0, 0.0};
                    if (kind >= 1) {
                        const double *w1 = V + LD * (s1 * nc + c);
                        const long long lrow = (long long)l1 * n;
#pragma unroll
                        for (int r = 0; r < 4; ++r) y[r] = pl_row_dot(p.ellt_val, p.ellt_col, (lrow + min(r0 + 4 * r, n - 1)) * etw, etw, w1);
                    }
                    if (kind == 2) {
                        const double *w2 = V + LD * (s2 * nc + c);
                        const long long lrow = (long long)l2 * n;
#pragma unroll
                        for (int r = 0; r < 4; ++r) y[r] = pl_row_dot(p.ellt_val, p.ellt_col, (lrow + min(r0 + 4 * r, n - 1)) * etw, etw, w2, y[r]);  // (onto the first term)
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rr = r0 + 4 * r;
                        if (rr < n) D[rr + LD * vc] = __builtin_fma(f, kind ? acc[r] + y[r] : acc[r], Y[rr + LD * vc]);
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
    // ---- behind the chain: f1 <- [G^T W | .], f2 <- [X_k | G X_k] --------------------------------------------------------------------------------
    const bool first = pr == 0;
    const int ctz = (nce + 15) >> 4;
    if (first) {
        for (int ct = 0; ct < ctz; ++ct) {
            const int vc = ct * 16 + li;
            const bool on = vc < nce;
            const double4_t acc = pl_tile(a, (on ? Y + LD * vc : G) + lk, kmask);
            if (on) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = rt * 16 + lk + 4 * r;
                    if (rr < n) f1[rr + LD * vc] = acc[r];
                }
            }
        }
    }
    for (int e = tid; e < nce * n; e += nth) {
        const int c = e / n, i = e - c * n;
        f2[i + LD * c] = zk[x_off + (c0 + c) * n + i];
    }
    __syncthreads();
    if (diag) {  // G X_k (A = G: the registers are reloaded), behind the nc columns of X_k
        kmask = pl_load_a<false>(G, LD, n, rt, li, lk, a);
        for (int ct = 0; ct < ctz; ++ct) {
            const int vc = ct * 16 + li;
            const bool on = vc < nce;
            const double4_t acc = pl_tile(a, (on ? f2 + LD * vc : G) + lk, kmask);
            if (on) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = rt * 16 + lk + 4 * r;
                    if (rr < n) f2[rr + LD * (nc + vc)] = acc[r];
                }
            }
        }
        __syncthreads();
    }
    // ---- partial sums, one wave per (column, entry): this unit's pairs | its drives' (dt,u_l) on the diagonal | (dt,dt) in unit (0,0) ------------------
    const int npair = m * (m + 1) / 2, nscal = (m + 1) * (m + 2) / 2;
    const int i0 = min(lane, n - 1), i1 = min(lane + 64, n - 1);  // the rows a lane takes (clamped: the loads stay legal)
    const bool ok0 = lane < n, ok1 = lane + 64 < n;
    double *ws = p.hpart + (item * d + c0) * nscal;
    const int ne = npb + (diag ? mgeI : 0) + (first ? 1 : 0);
    for (int pi = rt; pi < nce * ne; pi += nw) {
        const int c = pi / ne, t = pi - c * ne;
        const double *xc = f2 + LD * c, *gx = f2 + LD * (nc + c);
        double v;
        int o;
        if (t < npb) {
            int ai, bj;
            if (diag) {
                ai = 0;
                while ((ai + 1) * (ai + 2) / 2 <= t) ++ai;
                bj = t - ai * (ai + 1) / 2;
            } else {
                ai = t / mg;
                bj = t - ai * mg;
            }
            if (ai >= mgeI || bj >= mgeJ) continue;
            const double *w = Y + LD * ((1 + ndb + t) * nc + c);
            v = __builtin_fma(ok1 ? w[i1] : 0.0, xc[i1], (ok0 ? w[i0] : 0.0) * xc[i0]);
            const int i = lI + ai, l = lJ + bj;
            o = i * (i + 1) / 2 + l;
        } else if (t < npb + (diag ? mgeI : 0)) {
            const int ai = t - npb, l = lI + ai;
            const double *dw = Y + LD * ((1 + ai) * nc + c), *w = Y + LD * c;
            double y0 = 0.0, y1 = 0.0;  // (G_l X_k)[row]
            const long long e0 = ((long long)l * n + i0) * ew, e1 = ((long long)l * n + i1) * ew;
            for (int e = 0; e < ew; ++e) {
                y0 = __builtin_fma(p.ell_val[e0 + e], xc[p.ell_col[e0 + e]], y0);
                y1 = __builtin_fma(p.ell_val[e1 + e], xc[p.ell_col[e1 + e]], y1);
            }
            const double v0 = ok0 ? __builtin_fma(w[i0], y0, dw[i0] * gx[i0]) : 0.0;
            const double v1 = ok1 ? __builtin_fma(w[i1], y1, dw[i1] * gx[i1]) : 0.0;
            v = v0 + v1;
            o = npair + l;
        } else {
            const double *gw = f1 + LD * c;
            v = __builtin_fma(ok1 ? gw[i1] : 0.0, gx[i1], (ok0 ? gw[i0] : 0.0) * gx[i0]);
            o = npair + m;
        }
        v = wave_sum(v);
        if (lane == 0) ws[(long long)c * nscal + o] = -v;
    }
    // ---- the vectors: (u_l, X_k) from the diagonal units, (dt, X_k) from unit (0,0) ------------------------------------------------------------------
    double *H = p.hess + item * p.hess_per;
    double *H3 = H + nscal, *H4 = H3 + (long long)m * xd;
    if (diag)
        for (int e = tid; e < mgeI * nce * n; e += nth) {
            const int i = e % n, c = (e / n) % nce, t = e / (n * nce);
            H3[(long long)(lI + t) * xd + (long long)(c0 + c) * n + i] = -Y[i + LD * ((1 + t) * nc + c)];
        }
    if (first)
        for (int e = tid; e < nce * n; e += nth) H4[(long long)c0 * n + e] = -f1[(e % n) + LD * (e / n)];
}

// The scalar entries [(u_i,u_l), l <= i | (dt,u_l) | (dt,dt)] of every interval: the columns' partial sums added in column order, one thread per entry.
__global__ __launch_bounds__(256) void pcl_large_exp_hess_sum_kernel(const KParams p) {
    const int m = p.m, C = p.cols, nscal = (m + 1) * (m + 2) / 2;
    const long long item = blockIdx.x;
    const double *ws = p.hpart + item * C * nscal;
    double *H = p.hess + item * p.hess_per;
    for (int e = threadIdx.x; e < nscal; e += blockDim.x) {
        double t = 0.0;
        for (int c = 0; c < C; ++c) t += ws[(long long)c * nscal + e];
        H[e] = t;
    }
}

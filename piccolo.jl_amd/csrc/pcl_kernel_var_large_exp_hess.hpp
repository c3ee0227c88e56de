// Hessian of the Lagrangian on a large variational exponential context (PCL_BATCH_VARIATIONAL_EXP | PCL_LARGE_N | PCL_LARGE_VAR | PCL_LARGE_VAR_EXP,
// pade_order = PCL_ORDER_EXP, 66 <= n <= 128; option large_var_exp_hess): values, order and layout are those of the variational exponential context
// at n <= 62 with var_exp_hess (pcl_kernel_var_exp_hess.hpp) -- per interval the (m + 1)(m + 2) / 2 scalars [(u_i,u_l), l <= i | (dt,u_l) | (dt,dt)],
// then the vectors [(u_l, X'_k) | (dt, X'_k)] over the stacked, component-major state, nothing on X'_{k+1}.
//
// The formulation is the adjoint recurrence of pcl_kernel_large_exp_hess.hpp on the lifted generator Ghat = var_G(G, [Gv_b]) -- G on the diagonal
// blocks, Gv_b in block (b, 0), dGhat / du_l = I (x) G_l -- without a lifted matrix:
//       (Ghat^T W')_0 = G^T W_0 + sum_b Gv_b^T W_b,      (Ghat^T W')_b = G^T W_b,      (Ghat X')_b = G X_b + Gv_b X_0.
// A lifted product is the matrix-core product of the ONE tile G^T with the columns of every component plus a sparse row product with Gv_b^T read from
// memory, the shape of the drive terms.  s' = ceil(|h| |G(u_k)|_1) substeps from the n x n tile alone (the norm routine and the clamp of
// pcl_var_large_exp_kernel: the Jacobian launch of the same context takes the same substeps), degree LE_DEG, f = h_s / j, Horner for j = LE_DEG .. 1,
// every right-hand side on the columns from before the level's update; per component b of the stacked multipliers
//       d2W_b,il <- d2Y_b,il + f (G^T d2W_b,il + [b = 0] sum_c Gv_c^T d2W_c,il + G_i^T dW_b,l + G_l^T dW_b,i)
//       dW_b,l   <- dY_b,l   + f (G^T dW_b,l   + [b = 0] sum_c Gv_c^T dW_c,l   + G_l^T W_b)
//       W_b      <- Y_b      + f (G^T W_b      + [b = 0] sum_c Gv_c^T W_c)
// from Y' = M', dY = d2Y = 0.  After the last substep, with primes for the stacked quantities,
//       (u_i,u_l) = -sum_b <d2W_b,il, X_b>     (dt,u_l) = -<dW'_l, Ghat X'> - <W', (I (x) G_l) X'>     (dt,dt) = -<Ghat^T W', Ghat X'>
//       (u_l,X'_k) = -dW'_l                    (dt,X'_k) = -Ghat^T W'
// The third Frechet derivative that the octuple chain of pcl_kernel_var_exp_hess.hpp forms is carried implicitly by d2W_0.  h = 0: s' = 0, the (u,u)
// and (u,X') entries are exact zeros.
//
// PASSES.  The Lagrangian is linear in the multipliers, so the launch is the sum of 1 + v passes, each a unit (workgroup) of its own:
//   pass 0       the plain problem (M_0, X_0): one component, the operations of pcl_large_exp_hess_kernel in that kernel's order
//   pass b >= 1  the two components (0, b) under the multipliers (0, M_b): W_0, dW_0, d2W_0 start from zero and are fed through Gv_b^T alone
// Three rotating buffers of 9 columns are all the tile leaves at n = 128: an off-diagonal two-component unit of one drive per group takes
// 2 (1 + 2 + 1) = 8 of them, all 1 + v components at once would take 12.  With M_b = 0 for every b > 0 the later passes hold exact zeros: the scalars
// and the X_0 vectors are then, as numbers, those of a plain PCL_LARGE_N | PCL_LARGE_EXP context with large_exp_hess on (G0, Gj).
//
// Units: one workgroup per (interval, pass b, slice s of nc state columns, pair of drive groups (I, J), J <= I, of at most mg drives each), the unit
// index of pcl_large_exp_hess_kernel inside a pass.  A buffer column is (component slot cp, block bl, column c) at index cp T nc + bl nc + c with the
// blocks of that kernel (W | dW_I | dW_J off the diagonal | d2W; T = 1 + dW blocks + d2W blocks); slot 0 is component 0, slot 1 component b.
// LDS (doubles): G | three buffers of Wc columns | slack | us;  Wc = 2 nc T with the off-diagonal T wherever there is more than one group;
// no drives: 4 nc ([X_0 | X_b | (Ghat X')_0 | (Ghat X')_b] behind the chain).
//
// Determinism: no atomics.  A column's partial sums are formed by one wave per (column, entry), lanes over the rows, one shuffle tree per component,
// component 0 before component b, into the workspace p.hpart: [interval][pass][column][(m + 1)(m + 2) / 2]; every entry has exactly one writer.  The
// X_b vectors leave with pass b, the X_0 vectors of pass 0 too; what pass b >= 1 adds to the X_0 vectors goes to w.vpart:
// [interval][b - 1][m + 1][n cols].  pcl_var_large_exp_hess_sum_kernel (the same stream, behind this launch) adds the passes in the order 0, 1, ..,
// within a pass the columns in column order.  Every split (sx, mg) gives the same bits, and so do two launches.
//
// Truncation.  With A = h_s G, |A|_1 <= 1, the third derivative of the degree-18 polynomial misses at most sum_{k >= 16} 1 / k! < 5.1e-14 of
// |h_s Gv_b| |h_s G_i| |h_s G_l| per substep (DESIGN.md has what was read against the scipy truth).  The degree stays 18: pass 0's bits need it.
#pragma once

struct VarLargeExpHessParams {
    const double *gv_val;   // the variation generators row-compressed, [v][n][gv_w] (row-major, zero padded, columns ascending)
    const int *gv_col;
    const double *gvt_val;  // ... and their transposes, [v][n][gvt_w]
    const int *gvt_col;
    double *vpart;          // what the passes b >= 1 add to the X_0 vectors: [interval][b - 1][m + 1][n cols]
    int gv_w, gvt_w;
    int v;
    int xo[1 + PCL_VAR_MAXV];  // state offsets of the components in the knot
    int sx, mg, ngrp, Wc;      // slices per interval, drives per group, groups, columns per buffer
};

// p: Z, mu, hess, hpart, G0, upos / ucoef / n_upos (build_G), ell_* and ellt_* (the drives and their transposes), n, cols, m, K, z_dim, u_off,
// dt_off, LD, nc, lds_doubles, hess_per
__global__ __launch_bounds__(PL_NT) void pcl_var_large_exp_hess_kernel(const KParams p, const VarLargeExpHessParams w) {
    extern __shared__ double lds[];
    const int n = p.n, d = p.cols, m = p.m, LD = p.LD, nc = p.nc, v = w.v, sx = w.sx, mg = w.mg, ngrp = w.ngrp, Wc = w.Wc;
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, rt = tid >> 6, nw = nth >> 6;  // one wave per row tile
    const int li = lane & 15, lk = lane >> 4;
    const int npr = ngrp * (ngrp + 1) / 2, U = sx * npr;
    const long long bid = blockIdx.x;
    const long long kb = bid / U;  // (interval, pass)
    const int u = (int)(bid % U);
    const long long k = kb / (1 + v);
    const int b = (int)(kb % (1 + v));
    const int ncomp = b ? 2 : 1;
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
    const int T = 1 + ndb + npb, cx1 = T * nc, cx = ncomp * cx1;  // columns of a component; of the unit
    const double *zk = p.Z + k * p.z_dim;
    const double h = zk[p.dt_off];
    const long long xd = (long long)n * d, xdl = xd * (1 + v);
    const double *mu = p.mu + k * xdl + b * xd;  // M_b
    double *G = lds, *B0 = G + LD * n, *B1 = B0 + LD * Wc, *B2 = B1 + LD * Wc;
    double *us = B2 + LD * Wc + PL_SLACK;
    for (int e = tid; e < p.lds_doubles; e += nth) lds[e] = 0.0;
    __syncthreads();
    build_G(p, p.G0, zk, G, us);
    __syncthreads();
    // |G|_1 and s': the routine of pcl_var_large_exp_kernel and pcl_large_exp_hess_kernel (the column sums go through the third buffer)
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
    for (int e = tid; e < nce * n; e += nth) {  // Y_b = M_b in the last slot; Y_0 of a later pass, the dY and d2Y blocks stay zero
        const int c = e / n, i = e - c * n;
        B0[i + LD * ((ncomp - 1) * cx1 + c)] = mu[(long long)(c0 + c) * n + i];
    }
    __syncthreads();
    double *Y = B0, *f1 = B1, *f2 = B2;
    const int ct_n = (cx + 15) >> 4;
    const int etw = p.ellt_w, ew = p.ell_w, gw = w.gv_w, gtw = w.gvt_w;
    const long long trow = (long long)(b - 1) * n;  // the rows of Gv_b and of Gv_b^T (b > 0)
    for (int st = 0; st < sp; ++st) {
        double *V = Y, *D = f1, *O = f2;
        for (int j = LE_DEG; j >= 1; --j) {
            const double f = hs / j;
            for (int ct = 0; ct < ct_n; ++ct) {
                const int vc = ct * 16 + li;
                const int cp = min(vc / cx1, ncomp - 1), rem = vc - cp * cx1;
                const int bl = rem / nc, c = rem - bl * nc;
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
                    const double *Vc = V + LD * (cp * cx1);  // this component's blocks
                    double y[4] = {0.0, 0.0, 0.0, 0.0};
                    if (kind >= 1) {
                        const double *w1 = Vc + LD * (s1 * nc + c);
                        const long long lrow = (long long)l1 * n;
#pragma unroll
                        for (int r = 0; r < 4; ++r) y[r] = pl_row_dot(p.ellt_val, p.ellt_col, (lrow + min(r0 + 4 * r, n - 1)) * etw, etw, w1);
                    }
                    if (kind == 2) {
                        const double *w2 = Vc + LD * (s2 * nc + c);
                        const long long lrow = (long long)l2 * n;
#pragma unroll
                        for (int r = 0; r < 4; ++r) y[r] = pl_row_dot(p.ellt_val, p.ellt_col, (lrow + min(r0 + 4 * r, n - 1)) * etw, etw, w2, y[r]);  // (onto the first term)
                    }
                    double t4[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) t4[r] = kind ? acc[r] + y[r] : acc[r];
                    if (b && cp == 0) {  // component 0 of a later pass: fed by Gv_b^T against the same block and column of component b
                        const double *xb = V + LD * (cx1 + rem);
#pragma unroll
                        for (int r = 0; r < 4; ++r) t4[r] += pl_row_dot(w.gvt_val, w.gvt_col, (trow + min(r0 + 4 * r, n - 1)) * gtw, gtw, xb);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rr = r0 + 4 * r;
                        if (rr < n) D[rr + LD * vc] = __builtin_fma(f, t4[r], Y[rr + LD * vc]);
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
    // ---- behind the chain: f1 <- Ghat^T W' ([slot][c]), f2 <- [X_0 | X_b | (Ghat X')_0 | (Ghat X')_b] ---------------------------------------------------
    const bool first = pr == 0;
    const int cz = ncomp * nc, ctz = (cz + 15) >> 4;
    if (first) {
        for (int ct = 0; ct < ctz; ++ct) {
            const int vc = ct * 16 + li;
            const int cp = min(vc / nc, ncomp - 1), c = vc - cp * nc;
            const bool on = vc < cz && c < nce;
            const double4_t acc = pl_tile(a, (on ? Y + LD * (cp * cx1 + c) : G) + lk, kmask);
            if (on) {
                const int r0 = rt * 16 + lk;
                double t4[4] = {acc[0], acc[1], acc[2], acc[3]};
                if (b && cp == 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) t4[r] += pl_row_dot(w.gvt_val, w.gvt_col, (trow + min(r0 + 4 * r, n - 1)) * gtw, gtw, Y + LD * (cx1 + c));
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = r0 + 4 * r;
                    if (rr < n) f1[rr + LD * vc] = t4[r];
                }
            }
        }
    }
    for (int e = tid; e < ncomp * nce * n; e += nth) {
        const int cp = e / (nce * n), r = e - cp * nce * n, c = r / n, i = r - c * n;
        f2[i + LD * (cp * nc + c)] = zk[w.xo[cp ? b : 0] + (c0 + c) * n + i];
    }
    __syncthreads();
    if (diag) {  // Ghat X' (A = G: the registers are reloaded), behind the columns of X'
        kmask = pl_load_a<false>(G, LD, n, rt, li, lk, a);
        for (int ct = 0; ct < ctz; ++ct) {
            const int vc = ct * 16 + li;
            const int cp = min(vc / nc, ncomp - 1), c = vc - cp * nc;
            const bool on = vc < cz && c < nce;
            const double4_t acc = pl_tile(a, (on ? f2 + LD * vc : G) + lk, kmask);
            if (on) {
                const int r0 = rt * 16 + lk;
                double t4[4] = {acc[0], acc[1], acc[2], acc[3]};
                if (cp) {  // + Gv_b X_0
#pragma unroll
                    for (int r = 0; r < 4; ++r) t4[r] += pl_row_dot(w.gv_val, w.gv_col, (trow + min(r0 + 4 * r, n - 1)) * gw, gw, f2 + LD * c);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = r0 + 4 * r;
                    if (rr < n) f2[rr + LD * (cz + vc)] = t4[r];
                }
            }
        }
        __syncthreads();
    }
    // ---- partial sums, one wave per (column, entry): this unit's pairs | its drives' (dt,u_l) on the diagonal | (dt,dt) in unit (0,0) ------------------
    const int npair = m * (m + 1) / 2, nscal = (m + 1) * (m + 2) / 2;
    const int i0 = min(lane, n - 1), i1 = min(lane + 64, n - 1);  // the rows a lane takes (clamped: the loads stay legal)
    const bool ok0 = lane < n, ok1 = lane + 64 < n;
    double *ws = p.hpart + (kb * d + c0) * nscal;
    const int ne = npb + (diag ? mgeI : 0) + (first ? 1 : 0);
    for (int pi = rt; pi < nce * ne; pi += nw) {
        const int c = pi / ne, t = pi - c * ne;
        int o, ai = 0, bj = 0;
        if (t < npb) {
            if (diag) {
                while ((ai + 1) * (ai + 2) / 2 <= t) ++ai;
                bj = t - ai * (ai + 1) / 2;
            } else {
                ai = t / mg;
                bj = t - ai * mg;
            }
            if (ai >= mgeI || bj >= mgeJ) continue;
            const int i = lI + ai, l = lJ + bj;
            o = i * (i + 1) / 2 + l;
        } else if (t < npb + (diag ? mgeI : 0)) {
            ai = t - npb;
            o = npair + lI + ai;
        } else {
            o = npair + m;
        }
        double tot = 0.0;
        for (int cp = 0; cp < ncomp; ++cp) {  // component 0 before component b
            const double *Yc = Y + LD * (cp * cx1);
            const double *xc = f2 + LD * (cp * nc + c), *gx = f2 + LD * (cz + cp * nc + c);
            double vv;
            if (t < npb) {
                const double *wv = Yc + LD * ((1 + ndb + t) * nc + c);
                vv = __builtin_fma(ok1 ? wv[i1] : 0.0, xc[i1], (ok0 ? wv[i0] : 0.0) * xc[i0]);
            } else if (t < npb + (diag ? mgeI : 0)) {
                const int l = lI + ai;
                const double *dw = Yc + LD * ((1 + ai) * nc + c), *wv = Yc + LD * c;
                double y0 = 0.0, y1 = 0.0;  // (G_l X_cp)[row]
                const long long e0 = ((long long)l * n + i0) * ew, e1 = ((long long)l * n + i1) * ew;
                for (int e = 0; e < ew; ++e) {
                    y0 = __builtin_fma(p.ell_val[e0 + e], xc[p.ell_col[e0 + e]], y0);
                    y1 = __builtin_fma(p.ell_val[e1 + e], xc[p.ell_col[e1 + e]], y1);
                }
                const double v0 = ok0 ? __builtin_fma(wv[i0], y0, dw[i0] * gx[i0]) : 0.0;
                const double v1 = ok1 ? __builtin_fma(wv[i1], y1, dw[i1] * gx[i1]) : 0.0;
                vv = v0 + v1;
            } else {
                const double *gwv = f1 + LD * (cp * nc + c);
                vv = __builtin_fma(ok1 ? gwv[i1] : 0.0, gx[i1], (ok0 ? gwv[i0] : 0.0) * gx[i0]);
            }
            vv = wave_sum(vv);
            tot = cp ? tot + vv : vv;
        }
        if (lane == 0) ws[(long long)c * nscal + o] = -tot;
    }
    // ---- the vectors: (u_l, X'_k) from the diagonal units, (dt, X'_k) from unit (0,0); component b and pass 0's component 0 into the values, what a
    //      later pass adds to component 0 into w.vpart ------------------------------------------------------------------------------------------------
    double *H = p.hess + k * p.hess_per;
    double *H3 = H + nscal, *H4 = H3 + (long long)m * xdl;
    double *vp = b ? w.vpart + (k * v + (b - 1)) * (long long)(m + 1) * xd : nullptr;
    for (int cp = 0; cp < ncomp; ++cp) {
        const bool fed = b && cp == 0;
        double *o3 = fed ? vp : H3 + (long long)(cp ? b : 0) * xd, *o4 = fed ? vp + (long long)m * xd : H4 + (long long)(cp ? b : 0) * xd;
        const long long lstride = fed ? xd : xdl;
        if (diag)
            for (int e = tid; e < mgeI * nce * n; e += nth) {
                const int i = e % n, c = (e / n) % nce, t = e / (n * nce);
                o3[(long long)(lI + t) * lstride + (long long)(c0 + c) * n + i] = -Y[i + LD * (cp * cx1 + (1 + t) * nc + c)];
            }
        if (first)
            for (int e = tid; e < nce * n; e += nth) o4[(long long)c0 * n + e] = -f1[(e % n) + LD * (cp * nc + e / n)];
    }
}

// Behind the launch above, one workgroup per (interval, chunk): the scalar entries [(u_i,u_l), l <= i | (dt,u_l) | (dt,dt)] -- the passes in the order
// 0, 1, .., within a pass the columns' partial sums in column order, one thread per entry (chunk 0) -- and the X_0 vectors, onto which the passes
// b >= 1 are added in that order, one thread per element.
__global__ __launch_bounds__(256) void pcl_var_large_exp_hess_sum_kernel(const KParams p, const VarLargeExpHessParams w) {
    const int m = p.m, C = p.cols, v = w.v, nscal = (m + 1) * (m + 2) / 2;
    const long long k = blockIdx.x;
    const long long xd = (long long)p.n * C, xdl = xd * (1 + v);
    double *H = p.hess + k * p.hess_per;
    if (blockIdx.y == 0) {
        const double *ws = p.hpart + k * (1 + v) * C * nscal;
        for (int e = threadIdx.x; e < nscal; e += blockDim.x) {
            double t = 0.0;
            for (int bc = 0; bc < (1 + v) * C; ++bc) t += ws[(long long)bc * nscal + e];
            H[e] = t;
        }
    }
    const double *vp = w.vpart + k * v * (long long)(m + 1) * xd;
    for (long long e = (long long)blockIdx.y * blockDim.x + threadIdx.x; e < (m + 1) * xd; e += (long long)gridDim.y * blockDim.x) {
        const long long l = e / xd, q = e - l * xd;
        double t = H[nscal + l * xdl + q];
        for (int b = 0; b < v; ++b) t += vp[b * (long long)(m + 1) * xd + e];
        H[nscal + l * xdl + q] = t;
    }
}

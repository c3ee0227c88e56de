// Hessian of the Lagrangian on a large variational context (PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR, 66 <= n <= 128; option
// large_var_hess): values, order and layout are those of pcl_var_hess_kernel (pcl_kernel_variational.hpp) for the same system, at the diagonal
// Pade orders p = 2q (q <= 5).
//
// The formulation is that of pcl_kernel_pade_large_hess.hpp on the lifted generator Ghat = var_G(G, [Gv_b]) -- block lower triangular, G on the
// diagonal, Gv_b in block (b, 0), dGhat / du_l = I (x) G_l -- without ever forming a lifted matrix: a lifted product is the matrix-core product of
// the ONE tile G (or G^T) with the columns of every component, plus a sparse row product with Gv_b (Gv_b^T) read from memory, the shape of the
// drive terms.  With T_j = c_j h^j, Y_{b,j} = (-1)^j X_{b,k+1} - X_{b,k}:
//   forward:             Z_b <- G Z_b + [b > 0] Gv_b Z_0 + T_s Y_{b,s}
//   backward on Ghat^T:  W_0 <- G^T W_0 + sum_b Gv_b^T W_b,   W_b <- G^T W_b;   V_{l,.} the same pattern plus G_l^T W_.
//   scalars and vectors as in that file, per component.
// Three components do not fit beside the tile at n > 122, and the Lagrangian is linear in the multipliers, so a unit runs 1 + v PASSES:
//   pass 0       the plain Hessian of (M_0, X_0): the operations of pcl_pade_large_hess_kernel in their order
//   pass b >= 1  the two-component problem (X_0, X_b) with the multipliers (0, M_b) and Gv_b: W_0, V_{l,0} start from zero and are fed by
//                Gv_b^T W_b, Gv_b^T V_{l,b}; Z_0 is pass 0's (kept), Z_b is formed with the Gv_b Z_0 term
// The accumulators of the X_0 vectors and the per-column partial sums of the scalars stay in LDS over the passes; the X_b vectors are stored
// behind pass b.  With M_b = 0 for every b > 0 the later passes add exact zeros: the scalars and the X_0 vectors then carry the bits of a plain
// PCL_LARGE_N context with large_hess on (G0, Gj).
//
// Units: one workgroup per (interval, slice s of nc state columns, group g of mg drives), u = s + sx g, as in pcl_pade_large_hess_kernel; group 0
// stores the h vectors and the (h,h) partial sums.  Per state column the rows [F[i, 0 .. m-1] | (h,u_i)] go to p.hpart: [interval][column]
// [m (m + 1) + 1]; pcl_pade_large_hess_sum_kernel (the same stream, behind this launch) adds the columns in column order.
// LDS (doubles, LDc = LD nc), slot 0 = component 0, slot 1 = component b of the running pass:
//   G | per slot: -S, D, Z_1 .. Z_4 | X: per slot W | V_t (mg) | X' the same | per slot: A4, A6, A3_t (mg), A5_t (mg) | slack | us | sums
//   = 20 + 8 mg blocks per state column beside the tile (twice pcl_pade_large_hess_kernel's).
// Determinism: no atomics, no workgroup waits for another; every element and every partial sum is formed by one fixed sequence of operations
// that depends on (n, C, m, v, order) only -- the passes in the order 0, 1, .., v, within a pass component 0 before component b -- whatever the
// slice, the group or the device: every split gives the same bits, and so do two launches.
#pragma once

struct VarLargeHessParams {
    const double *gv_val;   // the variation generators row-compressed, [v][n][gv_w] (row-major, zero padded, columns ascending)
    const int *gv_col;
    const double *gvt_val;  // ... and their transposes, [v][n][gvt_w]
    const int *gvt_col;
    int gv_w, gvt_w;
    int v;
    int xo[1 + PCL_VAR_MAXV];  // state offsets of the components in the knot
    int sx, mg;                // state-column slices per interval, drives per group
};

// p: Z, mu, hess, hpart, G0, upos / ucoef / n_upos (build_G), ell_* and ellt_* (the drives and their transposes), n, cols, m, K, z_dim, u_off,
// dt_off, LD, nc, q, pc, lds_doubles, hess_per
__global__ __launch_bounds__(PL_NT) void pcl_var_large_hess_kernel(const KParams p, const VarLargeHessParams w) {
    extern __shared__ double lds[];
    const int n = p.n, d = p.cols, m = p.m, LD = p.LD, nc = p.nc, q = p.q, v = w.v, sx = w.sx, mg = w.mg;
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, rt = tid >> 6, nw = nth >> 6;  // one wave per row tile
    const int li = lane & 15, lk = lane >> 4;
    const int ngrp = m > 0 ? (m + mg - 1) / mg : 1, U = sx * ngrp;
    const long long bid = blockIdx.x;
    const long long k = bid / U;
    const int u = (int)(bid % U);
    const int s_ = u % sx, g = u / sx;
    const int c0 = s_ * nc, nce = max(0, min(nc, d - c0));             // this unit's state columns
    const int l0 = g * mg, mge = m > 0 ? max(0, min(mg, m - l0)) : 0;  // ... and drives
    const double *zk = p.Z + k * p.z_dim;
    const double *zn = zk + p.z_dim;
    const double h = zk[p.dt_off];
    const long long xd = (long long)n * d, xdl = xd * (1 + v);
    const double *mu = p.mu + k * xdl;
    const int LDc = LD * nc, CB = (1 + mg) * LDc, FB = 6 * LDc, AB = (2 + 2 * mg) * LDc;
    double *G = lds;
    double *Fw = G + LD * n;                    // per slot: -S | D | Z_1 .. Z_4 (Z_s at + (1 + s) LDc)
    double *Xc = Fw + 2 * FB, *Xn = Xc + 2 * CB;  // X: level s - 1, X': level s; per slot W | V_{l0} ..
    double *Ac = Xn + 2 * CB;                   // per slot: A4 | A6 | A3_t | A5_t
    double *us = Ac + 2 * AB + PL_SLACK;
    double *sacc = us + m + 8;               // [nc][mg][m + 1]: F[i, .] | (h,u_i) of this unit's columns and drives
    double *shh = sacc + nc * mg * (m + 1);  // [nc]: (h,h)
    for (int e = tid; e < p.lds_doubles; e += nth) lds[e] = 0.0;
    __syncthreads();
    build_G(p, p.G0, zk, G, us);
    const int ew = p.ell_w, etw = p.ellt_w, gw = w.gv_w, gtw = w.gvt_w;
    const int i0 = min(lane, n - 1), i1 = min(lane + 64, n - 1);  // the rows a lane takes in the sums (clamped: the loads stay legal)
    const bool ok0 = lane < n, ok1 = lane + 64 < n;
    const int nscal = (m + 1) * (m + 2) / 2, SW = m * (m + 1) + 1;
    double *H = p.hess + k * p.hess_per;
    double *H3 = H + nscal, *H4 = H3 + (long long)m * xdl, *H5 = H4 + xdl, *H6 = H5 + (long long)m * xdl;
    double a[PL_KS];
    for (int b = 0; b <= v; ++b) {
        const int sl = b ? 1 : 0, ncomp = 1 + sl;  // the slot this pass fills; the components it carries
        double *Sm = Fw + sl * FB, *Dm = Sm + LDc, *Zb = Dm + LDc;
        const double *Z0 = Fw + 2 * LDc;  // component 0's forward chain (pass 0's)
        if (b) {  // W_0 = 0, V = 0, and slot 1's accumulators start again
            for (int e = tid; e < 2 * CB; e += nth) Xc[e] = 0.0;
            for (int e = tid; e < AB; e += nth) Ac[AB + e] = 0.0;
            __syncthreads();
        }
        {
            const double Tq = p.pc[q] * plh_pow(h, q);
            const int xo = w.xo[b];
            for (int e = tid; e < nce * n; e += nth) {  // (columns beyond nce stay zero)
                const int c = e / n, i = e - c * n;
                const long long go = (long long)(c0 + c) * n + i;
                const double xn = zn[xo + go], xc = zk[xo + go];
                const double xs = xn + xc, xdv = xn - xc;
                const int idx = i + LD * c;
                Sm[idx] = -xs;
                Dm[idx] = xdv;
                if (q >= 2) Zb[(q - 2) * LDc + idx] = Tq * ((q & 1) ? -xs : xdv);
                Xc[sl * CB + idx] = mu[b * xd + go];  // W_0 of this component = M_b
            }
        }
        __syncthreads();
        // ---- forward chain of this pass's component: A = G ------------------------------------------------------------------------------------
        unsigned kmask = pl_load_a<false>(G, LD, n, rt, li, lk, a);
        const int ctz = (nc + 15) >> 4;
        for (int s = q - 2; s >= 1; --s) {  // Z_s = G Z_{s+1} + [b > 0] Gv_b Z_{0,s+1} + T_{s+1} Y_{s+1}
            const double *Ys = ((s + 1) & 1) ? Sm : Dm;
            const double Ts = p.pc[s + 1] * plh_pow(h, s + 1);
            const double *src = Zb + s * LDc;
            double *dst = Zb + (s - 1) * LDc;
            for (int ct = 0; ct < ctz; ++ct) {
                const int c = ct * 16 + li;
                const bool on = c < nce;
                const double4_t acc = pl_tile(a, (on ? src + LD * c : G) + lk, kmask);
                if (on) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rr = rt * 16 + lk + 4 * r;
                        double t = acc[r];
                        if (b) t = acc[r] + pl_row_dot(w.gv_val, w.gv_col, ((long long)(b - 1) * n + min(rr, n - 1)) * gw, gw, Z0 + s * LDc + LD * c);
                        if (rr < n) dst[rr + LD * c] = __builtin_fma(Ts, Ys[rr + LD * c], t);
                    }
                }
            }
            __syncthreads();
        }
        // ---- backward chains: A = G^T (the tile's columns) -------------------------------------------------------------------------------------
        kmask = pl_load_a<true>(G, LD, n, rt, li, lk, a);
        const int cb = (1 + mg) * nc, cx = ncomp * cb, ctn = (cx + 15) >> 4;
        const long long trow = (long long)(b - 1) * n;  // Gv_b^T's rows (b > 0)
        for (int s = 1; s <= q; ++s) {
            const double cs = p.pc[s], hp1 = plh_pow(h, s - 1), hm1 = plh_pow(-h, s - 1);
            const double Ts = cs * (hp1 * h), Tms = cs * (hm1 * -h), T1 = (s * cs) * hp1, T1m = (s * cs) * hm1;
            for (int ct = 0; ct < ctn; ++ct) {
                const int vc = ct * 16 + li;
                const int cp = min(vc / cb, ncomp - 1), rem = vc - cp * cb;  // slot, then block 0: W, 1 + t: V of drive l0 + t
                const int bl = rem / nc, c = rem - bl * nc;
                const bool on = vc < cx && c < nce && (bl == 0 || bl - 1 < mge);
                const double4_t acc = pl_tile(a, (on ? Xc + cp * CB + bl * LDc + LD * c : G) + lk, kmask);
                if (on) {
                    const int r0 = rt * 16 + lk;
                    const bool fed = b && cp == 0;  // component 0 of a later pass: fed by Gv_b^T (the same block and column of slot 1)
                    const double *xb = Xc + CB + bl * LDc + LD * c;
                    double *Xo = Xn + cp * CB, *A4 = Ac + cp * AB, *A6 = A4 + LDc, *A3 = A6 + LDc, *A5 = A3 + mg * LDc;
                    if (bl == 0) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int rr = r0 + 4 * r, idx = rr + LD * c;
                            double t = acc[r];
                            if (fed) t = acc[r] + pl_row_dot(w.gvt_val, w.gvt_col, (trow + min(rr, n - 1)) * gtw, gtw, xb);
                            if (rr < n) {
                                Xo[idx] = t;
                                A4[idx] = __builtin_fma(T1, t, A4[idx]);
                                A6[idx] = __builtin_fma(T1m, t, A6[idx]);
                            }
                        }
                    } else {
                        const int t = bl - 1;
                        const double *wc = Xc + cp * CB + LD * c;  // W_{s-1} of the same component
                        const long long lrow = (long long)(l0 + t) * n;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int rr = r0 + 4 * r, idx = rr + LD * c;
                            const double y = pl_row_dot(p.ellt_val, p.ellt_col, (lrow + min(rr, n - 1)) * etw, etw, wc);  // (G_l^T W_{s-1})[rr]
                            double vv = acc[r] + y;
                            if (fed) vv = vv + pl_row_dot(w.gvt_val, w.gvt_col, (trow + min(rr, n - 1)) * gtw, gtw, xb);
                            if (rr < n) {
                                Xo[bl * LDc + idx] = vv;
                                A3[t * LDc + idx] = __builtin_fma(Ts, vv, A3[t * LDc + idx]);
                                A5[t * LDc + idx] = __builtin_fma(Tms, vv, A5[t * LDc + idx]);
                            }
                        }
                    }
                }
            }
            __syncthreads();  // level s is complete in X'; the next level's products read it and write the other copy
            double *t_ = Xc;
            Xc = Xn;
            Xn = t_;
            // partial sums of level s, one wave per (column, entry), component 0 before component b: entry t < m: y = G_t Z_s (F[., t]);
            // t = m: y = Y_s ((h,u)); t = m + 1: (h,h)
            for (int pi = rt; pi < nce * (m + 2); pi += nw) {
                const int c = pi / (m + 2), t = pi - c * (m + 2);
                for (int cp = 0; cp < ncomp; ++cp) {
                    const double *Ys = Fw + cp * FB + ((s & 1) ? 0 : LDc);
                    const double *Zs = Fw + cp * FB + (1 + s) * LDc;
                    const double *Xp = Xc + cp * CB;
                    if (t == m + 1) {
                        if (g != 0 || s < 2) continue;
                        const double *wv = Xp + LD * c, *yc = Ys + LD * c;
                        double vv = __builtin_fma(ok1 ? wv[i1] : 0.0, yc[i1], (ok0 ? wv[i0] : 0.0) * yc[i0]);
                        vv = wave_sum(vv);
                        if (lane == 0) shh[c] = __builtin_fma((s * (s - 1) * cs) * plh_pow(h, s - 2), vv, shh[c]);
                        continue;
                    }
                    if (mge == 0 || (t < m && s >= q)) continue;
                    double y0 = 0.0, y1 = 0.0, coef = 1.0;
                    if (t < m) {
                        const double *zc = Zs + LD * c;
                        const long long e0 = ((long long)t * n + i0) * ew, e1 = ((long long)t * n + i1) * ew;
                        for (int e = 0; e < ew; ++e) {
                            y0 = __builtin_fma(p.ell_val[e0 + e], zc[p.ell_col[e0 + e]], y0);
                            y1 = __builtin_fma(p.ell_val[e1 + e], zc[p.ell_col[e1 + e]], y1);
                        }
                    } else {
                        y0 = Ys[i0 + LD * c];
                        y1 = Ys[i1 + LD * c];
                        coef = T1;
                    }
                    if (!ok0) y0 = 0.0;
                    if (!ok1) y1 = 0.0;
                    for (int ti = 0; ti < mge; ++ti) {
                        const double *vcol = Xp + (1 + ti) * LDc + LD * c;
                        double vv = __builtin_fma(vcol[i1], y1, vcol[i0] * y0);
                        vv = wave_sum(vv);
                        double *o = sacc + ((long long)(c * mg + ti) * (m + 1) + t);
                        if (lane == 0) *o = __builtin_fma(coef, vv, *o);
                    }
                }
            }
        }
        __syncthreads();
        // ---- the vectors of component b leave with their pass; component 0's behind the last one ----------------------------------------------
        for (int cp = (b == v ? 0 : 1); cp < ncomp; ++cp) {
            const double *A4 = Ac + cp * AB, *A6 = A4 + LDc, *A3 = A6 + LDc, *A5 = A3 + mg * LDc;
            const long long cofs = (long long)(cp ? b : 0) * xd;
            for (int e = tid; e < mge * nce * n; e += nth) {
                const int i = e % n, c = (e / n) % nce, t = e / (n * nce);
                const int idx = t * LDc + i + LD * c;
                const long long o = (long long)(l0 + t) * xdl + cofs + (long long)(c0 + c) * n + i;
                H3[o] = -A3[idx];
                H5[o] = A5[idx];
            }
            if (g == 0)
                for (int e = tid; e < nce * n; e += nth) {
                    const int idx = (e % n) + LD * (e / n);
                    const long long o = cofs + (long long)c0 * n + e;
                    H4[o] = -A4[idx];
                    H6[o] = -A6[idx];
                }
        }
        __syncthreads();  // (the next pass clears slot 1's accumulators)
    }
    double *ws = p.hpart + (k * d + c0) * SW;
    for (int e = tid; e < nce * mge * (m + 1); e += nth) {
        const int t = e % (m + 1), ti = (e / (m + 1)) % mge, c = e / ((m + 1) * mge);
        ws[(long long)c * SW + (l0 + ti) * (m + 1) + t] = sacc[(c * mg + ti) * (m + 1) + t];
    }
    if (g == 0)
        for (int c = tid; c < nce; c += nth) ws[(long long)c * SW + m * (m + 1)] = shh[c];
}

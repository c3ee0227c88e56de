// Hessian of the Lagrangian on a large context (PCL_LARGE_N, 66 <= n <= 128; option large_hess): values, order and layout are those of
// pcl_hess_general_kernel (pcl_kernels_hessian.hpp) for the same KParams, at the diagonal Pade orders p = 2q (q <= 5).
//
// The machinery is that of pcl_kernel_pade_large.hpp -- ONE n x n tile with LD = n | 1, one wave per 16-row tile with its MFMA A operand in
// registers over all levels (pl_tile: four accumulators summed in one fixed order, a wave-uniform mask over empty 16 x 4 blocks, zero-filled LDS
// and PL_SLACK doubles so that the unconditional B operand loads are legal), the drives' ELL rows read from memory -- on a formulation without
// the m (m + 1) / 2 blocks U_il of the general kernel.  With T_j = c_j h^j, Y_j = (-1)^j X_{k+1} - X_k, M = mu_k:
//   forward (A = G, independent of the drives):   Z_{q-1} = T_q Y_q,   Z_{s-1} = G Z_s + T_s Y_s          (Z_s = sum_{j > s} T_j G^(j-s-1) Y_j)
//   backward (A = G^T: the tile's columns; the A registers are reloaded), s = 1 .. q:
//                                                 W_s = G^T W_{s-1} (W_0 = M),   V_{l,s} = G^T V_{l,s-1} + G_l^T W_{s-1} (V_{l,0} = 0)
//   F[i,l] = sum_{s < q} <V_{i,s}, G_l Z_s>  (G_l Z_s formed on the fly from the ELL rows),   (u_i,u_l) = F[i,l] + F[l,i]
//   (h,u_l) = sum_s s c_s h^(s-1) <V_{l,s}, Y_s>,   (h,h) = sum_{s >= 2} s (s-1) c_s h^(s-2) <W_s, Y_s>
//   d2/du_l dX_k = -sum_s T_s V_{l,s},  d2/dh dX_k = -sum_s s c_s h^(s-1) W_s,  d2/du_l dX_{k+1} = sum_s c_s (-h)^s V_{l,s},  d2/dh dX_{k+1} = -sum_s s c_s (-h)^(s-1) W_s
// Dense products per unit and state column: (q - 2) + q (1 + mg).
//
// Units: one workgroup per (interval, slice s of nc state columns, group g of mg drives): u = s + sx g.  Every group forms Z and W with the
// same operations (the same bits); group 0 stores the h vectors and the (h,h) partial sums; every group stores the vectors of its drives and,
// per state column, the rows [F[i, 0 .. m-1] | (h,u_i)] of its drives into the workspace p.hpart: [interval][column][m (m + 1) + 1] doubles.
// pcl_pade_large_hess_sum_kernel (the same stream, behind this launch) adds the columns in column order into the (m + 1)(m + 2) / 2 scalars.
// LDS (doubles, LDc = LD nc): G | -S | D | Z_1 .. Z_4 | X = W | V_t (1 + mg) | X' | A4 | A6 | A3_t (mg) | A5_t (mg) | slack | us | sums
//   = 10 + 4 mg blocks per state column beside the tile; the vector outputs accumulate in A3 .. A6, each element by the lane that forms it.
// Determinism: no atomics; a column's partial sums are formed by one wave per (column, entry) -- lanes over the rows, one shuffle tree, the
// levels added in order -- whatever the slice or the group, and the columns are added in order by the second launch: every split gives the
// same bits, and so do two launches.
#pragma once

#define PLH_ZB 4  // blocks of the forward chain: Z_1 .. Z_{q-1}, q <= 5

__device__ __forceinline__ double plh_pow(double x, int j) {
    double r = 1.0;
    for (int i = 0; i < j; ++i) r *= x;
    return r;
}

// p.nc state columns per slice, p.lds_doubles to zero-fill; sx slices, mg drives per group
__global__ __launch_bounds__(PL_NT) void pcl_pade_large_hess_kernel(const KParams p, const int sx, const int mg) {
    extern __shared__ double lds[];
    const int n = p.n, d = p.cols, m = p.m, LD = p.LD, nc = p.nc, q = p.q;
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, rt = tid >> 6, nw = nth >> 6;  // one wave per row tile
    const int li = lane & 15, lk = lane >> 4;
    const int ngrp = m > 0 ? (m + mg - 1) / mg : 1, U = sx * ngrp;
    const long long bid = blockIdx.x;
    const long long item = bid / U;
    const int u = (int)(bid % U);
    const int k = (int)(item % p.K), b = (int)(item / p.K);
    const int s_ = u % sx, g = u / sx;
    const int c0 = s_ * nc, nce = max(0, min(nc, d - c0));          // this unit's state columns
    const int l0 = g * mg, mge = m > 0 ? max(0, min(mg, m - l0)) : 0;  // ... and drives
    const double *zk = p.Z + (long long)b * p.z_batch_stride + (long long)k * p.z_dim;
    const double *zn = zk + p.z_dim;
    const double h = zk[p.dt_off];
    const long long xd = (long long)n * d;
    const double *mu = p.mu + item * xd;
    const int LDc = LD * nc;
    double *G = lds;
    double *Sm = G + LD * n, *Dm = Sm + LDc, *Zb = Dm + LDc;  // Z_s at Zb + (s - 1) LDc
    double *Xc = Zb + PLH_ZB * LDc, *Xn = Xc + (1 + mg) * LDc;  // X: W | V_{l0} .. (level s - 1), X': level s
    double *A4 = Xn + (1 + mg) * LDc, *A6 = A4 + LDc, *A3 = A6 + LDc, *A5 = A3 + mg * LDc;
    double *us = A5 + mg * LDc + PL_SLACK;
    double *sacc = us + m + 8;                        // [nc][mg][m + 1]: F[i, .] | (h,u_i) of this unit's columns and drives
    double *shh = sacc + nc * mg * (m + 1);           // [nc]: (h,h)
    for (int e = tid; e < p.lds_doubles; e += nth) lds[e] = 0.0;
    __syncthreads();
    const int x_off = p.x_offs[p.z_batch_stride ? 0 : b];
    build_G(p, p.G0 + (long long)b * p.g0_batch_stride, zk, G, us);
    {
        const double Tq = p.pc[q] * plh_pow(h, q);
        for (int e = tid; e < nce * n; e += nth) {  // (columns beyond nce stay zero)
            const int c = e / n, i = e - c * n;
            const long long go = (long long)(c0 + c) * n + i;
            const double xn = zn[x_off + go], xc = zk[x_off + go];
            const double xs = xn + xc, xdv = xn - xc;
            const int idx = i + LD * c;
            Sm[idx] = -xs;
            Dm[idx] = xdv;
            if (q >= 2) Zb[(q - 2) * LDc + idx] = Tq * ((q & 1) ? -xs : xdv);
            Xc[idx] = mu[go];  // W_0 = M
        }
    }
    __syncthreads();
    double a[PL_KS];
    // ---- forward chain: A = G -----------------------------------------------------------------------------------------------------------
    unsigned kmask = pl_load_a<false>(G, LD, n, rt, li, lk, a);
    const int ctz = (nc + 15) >> 4;
    for (int s = q - 2; s >= 1; --s) {  // Z_s = G Z_{s+1} + T_{s+1} Y_{s+1}
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
                    if (rr < n) dst[rr + LD * c] = __builtin_fma(Ts, Ys[rr + LD * c], acc[r]);
                }
            }
        }
        __syncthreads();
    }
    // ---- backward chains: A = G^T (the tile's columns) -------------------------------------------------------------------------------------
    kmask = pl_load_a<true>(G, LD, n, rt, li, lk, a);
    const int cx = (1 + mg) * nc, ctn = (cx + 15) >> 4;
    const int ew = p.ell_w, etw = p.ellt_w;
    const int i0 = min(lane, n - 1), i1 = min(lane + 64, n - 1);  // the rows a lane takes in the sums (clamped: the loads stay legal)
    const bool ok0 = lane < n, ok1 = lane + 64 < n;
    for (int s = 1; s <= q; ++s) {
        const double cs = p.pc[s], hp1 = plh_pow(h, s - 1), hm1 = plh_pow(-h, s - 1);
        const double Ts = cs * (hp1 * h), Tms = cs * (hm1 * -h), T1 = (s * cs) * hp1, T1m = (s * cs) * hm1;
        for (int ct = 0; ct < ctn; ++ct) {
            const int vc = ct * 16 + li;
            const int bl = vc / nc, c = vc - bl * nc;  // block 0: W, 1 + t: V of drive l0 + t
            const bool on = vc < cx && c < nce && (bl == 0 || bl - 1 < mge);
            const double4_t acc = pl_tile(a, (on ? Xc + bl * LDc + LD * c : G) + lk, kmask);
            if (on) {
                const int r0 = rt * 16 + lk;
                if (bl == 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rr = r0 + 4 * r, idx = rr + LD * c;
                        if (rr < n) {
                            Xn[idx] = acc[r];
                            A4[idx] = __builtin_fma(T1, acc[r], A4[idx]);
                            A6[idx] = __builtin_fma(T1m, acc[r], A6[idx]);
                        }
                    }
                } else {
                    const int t = bl - 1;
                    const double *wc = Xc + LD * c;  // W_{s-1}
                    const long long lrow = (long long)(l0 + t) * n;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rr = r0 + 4 * r, idx = rr + LD * c;
                        // pl_row_dot's loop, open here: through the helper the compiler reads the table pointers ahead of the loop guard,
                        // and this kernel's launches measured slower.  The same operations in the same order
                        const long long eb = (lrow + min(rr, n - 1)) * etw;
                        double y = 0.0;  // (G_l^T W_{s-1})[rr]
                        for (int e = 0; e < etw; ++e) y = __builtin_fma(p.ellt_val[eb + e], wc[p.ellt_col[eb + e]], y);
                        const double v = acc[r] + y;
                        if (rr < n) {
                            Xn[bl * LDc + idx] = v;
                            A3[t * LDc + idx] = __builtin_fma(Ts, v, A3[t * LDc + idx]);
                            A5[t * LDc + idx] = __builtin_fma(Tms, v, A5[t * LDc + idx]);
                        }
                    }
                }
            }
        }
        __syncthreads();  // level s is complete in X'; the next level's products read it and write the other copy
        double *t_ = Xc;
        Xc = Xn;
        Xn = t_;
        // partial sums of level s, one wave per (column, entry): entry t < m: y = G_t Z_s (F[., t]); t = m: y = Y_s ((h,u)); t = m + 1: (h,h)
        const double *Ys = (s & 1) ? Sm : Dm;
        const double *Zs = Zb + (s - 1) * LDc;
        for (int pi = rt; pi < nce * (m + 2); pi += nw) {
            const int c = pi / (m + 2), t = pi - c * (m + 2);
            if (t == m + 1) {
                if (g != 0 || s < 2) continue;
                const double *w = Xc + LD * c, *yc = Ys + LD * c;
                double v = __builtin_fma(ok1 ? w[i1] : 0.0, yc[i1], (ok0 ? w[i0] : 0.0) * yc[i0]);
                v = wave_sum(v);
                if (lane == 0) shh[c] = __builtin_fma((s * (s - 1) * cs) * plh_pow(h, s - 2), v, shh[c]);
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
                const double *vcol = Xc + (1 + ti) * LDc + LD * c;
                double v = __builtin_fma(vcol[i1], y1, vcol[i0] * y0);
                v = wave_sum(v);
                double *o = sacc + ((long long)(c * mg + ti) * (m + 1) + t);
                if (lane == 0) *o = __builtin_fma(coef, v, *o);
            }
        }
    }
    __syncthreads();
    // ---- stores ----------------------------------------------------------------------------------------------------------------------------
    const int nscal = (m + 1) * (m + 2) / 2, SW = m * (m + 1) + 1;
    double *H = p.hess + item * p.hess_per;
    double *H3 = H + nscal, *H4 = H3 + (long long)m * xd, *H5 = H4 + xd, *H6 = H5 + (long long)m * xd;
    for (int e = tid; e < mge * nce * n; e += nth) {
        const int i = e % n, c = (e / n) % nce, t = e / (n * nce);
        const int idx = t * LDc + i + LD * c;
        const long long o = (long long)(l0 + t) * xd + (long long)(c0 + c) * n + i;
        H3[o] = -A3[idx];
        H5[o] = A5[idx];
    }
    if (g == 0)
        for (int e = tid; e < nce * n; e += nth) {
            const int idx = (e % n) + LD * (e / n);
            const long long o = (long long)c0 * n + e;
            H4[o] = -A4[idx];
            H6[o] = -A6[idx];
        }
    double *ws = p.hpart + (item * d + c0) * SW;
    for (int e = tid; e < nce * mge * (m + 1); e += nth) {
        const int t = e % (m + 1), ti = (e / (m + 1)) % mge, c = e / ((m + 1) * mge);
        ws[(long long)c * SW + (l0 + ti) * (m + 1) + t] = sacc[(c * mg + ti) * (m + 1) + t];
    }
    if (g == 0)
        for (int c = tid; c < nce; c += nth) ws[(long long)c * SW + m * (m + 1)] = shh[c];
}

// The scalar entries [uu (i, l <= i) | hu | hh] of every interval: the columns' partial sums added in column order, one thread per entry.
__global__ __launch_bounds__(256) void pcl_pade_large_hess_sum_kernel(const KParams p) {
    const int m = p.m, C = p.cols, SW = m * (m + 1) + 1;
    const int npair = m * (m + 1) / 2, nscal = (m + 1) * (m + 2) / 2;
    const long long item = blockIdx.x;
    const double *ws = p.hpart + item * C * SW;
    double *H = p.hess + item * p.hess_per;
    for (int e = threadIdx.x; e < nscal; e += blockDim.x) {
        int o1, o2 = -1;
        if (e < npair) {
            int i = 0;
            while ((i + 1) * (i + 2) / 2 <= e) ++i;  // e = i (i + 1) / 2 + l, l <= i
            const int l = e - i * (i + 1) / 2;
            o1 = i * (m + 1) + l;
            o2 = l * (m + 1) + i;
        } else if (e < npair + m)
            o1 = (e - npair) * (m + 1) + m;
        else
            o1 = m * (m + 1);
        double t = 0.0;
        for (int c = 0; c < C; ++c) {
            const double *w = ws + (long long)c * SW;
            t += o2 >= 0 ? w[o1] + w[o2] : w[o1];
        }
        H[e] = t;
    }
}

// Large variational exponential kernel (contexts created with PCL_BATCH_VARIATIONAL_EXP | PCL_LARGE_N | PCL_LARGE_VAR | PCL_LARGE_VAR_EXP and
// pade_order = PCL_ORDER_EXP, 66 <= n <= 128): residual, and residual + exact Jacobian, of the exponential constraint on the lifted generator,
//     delta_0 = X_{k+1} - E X_k,      delta_i = Xv_{i,k+1} - (E Xv_{i,k} + L_i X_k),
// E = exp(h G(u_k)), L_i the Frechet derivative of exp at h G along h Gv_i.  Outputs, value order and layout are those of pcl_var_exp_kernel
// (pcl_kernel_var_exp.hpp): per interval -E (C copies); per variation -E, then -L_i; the ones of knot k + 1; the tails, component-major, per state
// column the m drive slices then the dt slice.
//
// ONE n x n tile fits (LD = n | 1), so this is the substepped degree-18 Taylor polynomial of pcl_kernel_large_exp.hpp in action form, on the lifted
// pair of pcl_kernel_var_large_rollout.hpp, with the drive derivative carried through both; the lifted matrix is never formed.
// s' = ceil(|h| |G(u_k)|_1) substeps of h_s = h / s', from the tile of G alone and clamped at LR_SMAX: every unit of an interval, and a plain large
// exponential context, takes the same substeps.  Per substep, Horner for j = LR_DEG .. 1 with f = h_s / j, every right-hand side on the columns
// from before this level's update:
//       dVv_il <- dYv_il + f ((G dVv_il + Gv_i dV_l) + G_l Vv_i)
//       dV_l   <- dY_l   + f (G dV_l + G_l V)
//       Vv_i   <- Yv_i   + f (G Vv_i + Gv_i V)
//       V      <- Y      + f  G V
// from Y = X_k, Yv_i = Xv_{i,k}, dY = dYv = 0.  After the last substep delta_0 = X_{k+1} - Y, delta_i = Xv_{i,k+1} - Yv_i; the drive tails are
// -dY_l and -dYv_il (-L_l X_k and -(L2_il X_k + L_l Xv_{i,k}), L2 the second Frechet derivative); the dt tails are -G Y and -(G Yv_i + Gv_i Y);
// -E and -L_i are the (V, Vv_i) recurrence on column panels of the identity with Yv = 0.  h = 0: s' = 0, E = I exactly, L_i, L2 and the drive
// tails exact zeros, component i's dt tail -(G Xv_i + Gv_i X).  A negative h is an ordinary step.
//
// A column of a buffer is (slot t, component b, column c) at index (t (1 + v) + b) ncu + c: slot 0 the values, slot 1 + j the derivative along the
// unit's drive j.  Its level is ONE expression,
//       y = G col                                  matrix-core column tile, the wave's rows of G in registers (pl_tile)
//       y += Gv_b (slot t, component 0, c)         b > 0: the row-compressed Gv_b against the old column in LDS (pl_row_dot)
//       y += G_l (slot 0, component b, c)          t > 0: the drive's ELL row against the old column in LDS (pl_row_dot)
//       new = fma(f, y, Y col)
// so component 0 takes the operations of pcl_large_exp_kernel in its order (the bits of a plain PCL_LARGE_N | PCL_LARGE_EXP context on the same
// drift and drives: delta_0, every copy of -E, its tails), and with Gv_i = 0 component i takes them on Xv_i.
//
// Units, one workgroup each, U per interval.  Chain unit u < sx ngrp: state-column slice s = u % sx (nc columns), drive group g = u / sx (mg
// drives), ALL 1 + v components: (1 + v) nc (1 + mg) columns.  Every group forms the value slot again with the same operations; group 0 stores
// delta, the ones and the dt tails, every group the tails of its drives.  Panel unit: npc columns of the identity, all components, no drives:
// (1 + v) npc columns; it stores -E to the 1 + v diagonal blocks and -L_i, C copies each.  The residual-only launch has chain units of the value
// slot alone.  The left factors are constant through the loop, so every column is independent: no sum crosses a unit, no atomics, no scratch.
// LDS (doubles): G | three buffers of W columns (Y, V, the level's result; they rotate) | slack | us.
//
// Truncation (|h_s G|_1 <= 1): value and first derivatives as in pcl_kernel_large_exp.hpp (8.7e-18, 1.6e-16 per substep).  The second
// derivative of the polynomial misses sum_{j >= 19} d2(A^j) / j!, |d2(A^j)| <= j (j - 1) |A|^{j-2} |dA_1| |dA_2|: at most
// sum_{j >= 19} 1 / (j - 2)! = sum_{k >= 17} 1 / k! < 3.0e-15 of |h_s Gv_i|_1 |h_s G_l|_1 per substep -- above 2^-53, and s' multiplies it
// (1.5e-13 at s' = 51), two decades inside the 1e-11 rule.  The degree stays 18: another one would break component 0's bits.
// Every element of every output is formed by one fixed sequence of operations whatever the split (sx, mg, npc): every split, repeated launches and
// both pointer paths give the same bits, and the residual-only delta has the bits of the fused launch's.
#pragma once

// p: Z, delta, jac, G0, upos / ucoef / n_upos (build_G), ell_* (the drives), n, cols, m, K, z_dim, u_off, dt_off, jac_per, LD, nc, S = units per
// interval, nt, lds_doubles; w: gv_val / gv_col / gv_w, v, xo, sx, mg, ngrp, npc, pu (Gv is not read)
template <bool JAC>
__global__ __launch_bounds__(PL_NT) void pcl_var_large_exp_kernel(const KParams p, const VarLargeParams w) {
    extern __shared__ double lds[];
    const int n = p.n, d = p.cols, m = p.m, LD = p.LD, U = p.S, v = w.v, comp = 1 + v;
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, rt = tid >> 6;  // one wave per row tile
    const int li = lane & 15, lk = lane >> 4;
    const long long bid = blockIdx.x;
    const long long k = bid / U;
    const int u = (int)(bid % U);
    const double *zk = p.Z + k * p.z_dim;
    const double *zn = zk + p.z_dim;
    const double h = zk[p.dt_off];
    const long long nn = (long long)n * n;
    const int nchain = w.sx * w.ngrp;
    const bool chain = u < nchain;
    const int g = chain ? u / w.sx : 0;
    const int ncu = chain ? p.nc : w.npc;                                                  // columns per component of this unit
    const int c0 = (chain ? u % w.sx : u - nchain) * ncu;                                  // ... the first of them (a state column | a column of E)
    const int nce = max(0, min(ncu, (chain ? d : n) - c0));
    const int mgu = (JAC && chain) ? w.mg : 0, l0 = g * mgu, mge = max(0, min(mgu, m - l0));  // this unit's drives
    const int CB = comp * ncu, cx = CB * (1 + mgu);                                        // columns of a slot; of the unit
    const int W = max(comp * p.nc * (JAC ? 1 + w.mg : 1), JAC ? comp * w.npc : 0);         // columns of a buffer (the host's count)
    double *G = lds, *B0 = G + LD * n, *B1 = B0 + LD * W, *B2 = B1 + LD * W;
    double *us = B2 + LD * W + PL_SLACK;
    for (int e = tid; e < p.lds_doubles; e += nth) lds[e] = 0.0;
    __syncthreads();
    build_G(p, p.G0, zk, G, us);
    __syncthreads();
    // |G|_1 as pcl_large_exp_kernel forms it: the column sums go through the third buffer (n <= LD W doubles; read back before anything else is written there)
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
    __syncthreads();  // (the norms have been read)
    if (tid < n) B2[tid] = 0.0;
    if (chain) {  // Y = X_k, Yv_i = Xv_{i,k}; the derivative slots stay zero
        for (int e = tid; e < comp * nce * n; e += nth) {
            const int b = e / (nce * n), r = e - b * nce * n, c = r / n, i = r - c * n;
            B0[i + LD * (b * ncu + c)] = zk[w.xo[b] + (c0 + c) * n + i];
        }
    } else {  // the panel of the identity; Yv = 0
        for (int e = tid; e < nce * n; e += nth) {
            const int c = e / n, i = e - c * n;
            B0[i + LD * c] = (i == c0 + c) ? 1.0 : 0.0;
        }
    }
    __syncthreads();
    double *Y = B0, *f1 = B1, *f2 = B2;
    const int ct_n = (cx + 15) >> 4;
    const int ew = p.ell_w, gw = w.gv_w;
    for (int st = 0; st < sp; ++st) {
        double *V = Y, *D = f1, *O = f2;
        for (int j = LR_DEG; j >= 1; --j) {
            const double f = hs / j;
            for (int ct = 0; ct < ct_n; ++ct) {
                const int vc = ct * 16 + li;
                const int t = vc / CB, rem = vc - t * CB, b = rem / ncu, c = rem - b * ncu;
                const bool on = vc < cx && c < nce && (t == 0 || t - 1 < mge);
                const double4_t acc = pl_tile(a, (on ? V + LD * vc : G) + lk, kmask);
                if (on) {
                    const int r0 = rt * 16 + lk;
                    double y[4] = {acc[0], acc[1], acc[2], acc[3]};
                    // (rows beyond n - 1 read the last row; the stores are predicated)
                    if (b > 0) {  // Gv_b V | Gv_b dV_l, with the column before this level's update
                        const double *xc = V + LD * (t * CB + c);
                        const long long vrow = (long long)(b - 1) * n;
#pragma unroll
                        for (int r = 0; r < 4; ++r) y[r] += pl_row_dot(w.gv_val, w.gv_col, (vrow + min(r0 + 4 * r, n - 1)) * gw, gw, xc);
                    }
                    if (t > 0) {  // G_l V | G_l Vv_b, likewise
                        const double *xc = V + LD * (b * ncu + c);
                        const long long lrow = (long long)(l0 + t - 1) * n;
#pragma unroll
                        for (int r = 0; r < 4; ++r) y[r] += pl_row_dot(p.ell_val, p.ell_col, (lrow + min(r0 + 4 * r, n - 1)) * ew, ew, xc);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rr = r0 + 4 * r;
                        if (rr < n) D[rr + LD * vc] = __builtin_fma(f, y[r], Y[rr + LD * vc]);
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
    const bool first = chain && g == 0;
    if (JAC && first) {  // the dt tails: G Y | G Yv_b + Gv_b Y into the free buffer (the sign goes on with the store)
        for (int ct = 0; ct < (CB + 15) >> 4; ++ct) {
            const int vc = ct * 16 + li;
            const int b = vc / ncu, c = vc - b * ncu;
            const bool on = vc < CB && c < nce;
            const double4_t acc = pl_tile(a, (on ? Y + LD * vc : G) + lk, kmask);
            if (on) {
                const int r0 = rt * 16 + lk;
                double y[4] = {acc[0], acc[1], acc[2], acc[3]};
                if (b > 0) {
                    const long long vrow = (long long)(b - 1) * n;
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[r] += pl_row_dot(w.gv_val, w.gv_col, (vrow + min(r0 + 4 * r, n - 1)) * gw, gw, Y + LD * c);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = r0 + 4 * r;
                    if (rr < n) f1[rr + LD * vc] = y[r];
                }
            }
        }
        __syncthreads();
    }
    const long long xdc = (long long)n * d, xdl = xdc * comp;
    if (p.delta && first)
        for (int e = tid; e < comp * nce * n; e += nth) {
            const int b = e / (nce * n), r = e - b * nce * n, c = r / n, i = r - c * n;
            p.delta[k * xdl + b * xdc + (long long)(c0 + c) * n + i] = zn[w.xo[b] + (c0 + c) * n + i] - Y[i + LD * (b * ncu + c)];
        }
    if (!JAC) return;
    double *jb = p.jac + k * p.jac_per;
    const long long blk = (long long)d * nn;  // one block of the values: C copies of an n x n matrix
    if (chain) {
        // d delta / d X'_{k+1} = I: its diagonal, from the unit that has the column
        double *jo = jb + (1 + 2 * v) * blk;
        if (first)
            for (int e = tid; e < comp * nce * n; e += nth) {
                const int b = e / (nce * n), r = e - b * nce * n;
                jo[b * xdc + (long long)c0 * n + r] = 1.0;
            }
        // tails [b][c][l | dt][i]: this group's drives, and the dt slice from group 0
        double *jt = jo + xdl;
        const int nl = mge + (first ? 1 : 0);
        for (int e = tid; e < comp * nce * nl * n; e += nth) {
            const int i = e % n, t = (e / n) % nl, c = (e / (n * nl)) % nce, b = e / (n * nl * nce);
            const int l = t < mge ? l0 + t : m;
            const double val = t < mge ? Y[i + LD * ((1 + t) * CB + b * ncu + c)] : f1[i + LD * (b * ncu + c)];
            jt[(((long long)b * d + c0 + c) * (m + 1) + l) * n + i] = -val;
        }
        return;
    }
    // -E into block 0 and the diagonal block 2 b - 1 of every variation, -L_b into block 2 b: this unit's panel, C copies each (n is even)
    const int hn = n >> 1;
    const bool pair = !(reinterpret_cast<unsigned long long>(jb) & 15ull);
    for (int e = tid; e < comp * nce * hn; e += nth) {
        const int b = e / (nce * hn), r = e - b * nce * hn, c = r / hn, i = 2 * (r - c * hn);
        const double *src = Y + LD * (b * ncu + c);
        const double v0 = -src[i], v1 = -src[i + 1];
        const int nplace = b ? 1 : comp;
        for (int pl = 0; pl < nplace; ++pl) {
            double *o = jb + (b ? 2 * b : (pl ? 2 * pl - 1 : 0)) * blk + (long long)(c0 + c) * n + i;
            for (int cc = 0; cc < d; ++cc) {
                if (pair)
                    store2(o + cc * nn, v0, v1, p.nt);
                else
                    o[cc * nn] = v0, o[cc * nn + 1] = v1;
            }
        }
    }
}

// pcl_kernels_objective.hpp -- terminal objectives in one general form, and the Hessian of the whole objective.
//
// Every terminal loss of the reference is  Q |1 - F(x)|  with F at most quadratic in the terminal state(s):
//     F(x) = c' x + sum_r (A_r' x)^2
//   KetInfidelityObjective                      F = |<g|psi>|^2                          2 rows          objectives.jl:24-60
//   CoherentKetInfidelityObjective              F = |sum_i w_i <g_i|psi_i> / sum w|^2    2 rows, JOINT   objectives.jl:96-200
//   DensityMatrix[PureState]InfidelityObjective F = Re tr(rho rho_goal)                  linear          objectives.jl:387-435
//   UnitaryInfidelityObjective                  F = |tr(G'U)|^2 / d^2                    2 rows          objectives.jl:330-337
//     ... with an EmbeddedOperator goal         F = (|M|_F^2 + |tr M|^2) / (ns (ns+1))   2 ns^2 + 2 rows objectives.jl:339-345
// (the rows are built on the host: pcl_set_goal_form, and by pcl_set_goal / pcl_set_goal_subspace for the Hessian of the unitary losses).
// x is one member's terminal state (scope 0: one term per member / seed, weights w_b) or the terminal states of all members
// concatenated in member order (scope 1: one term).  The absolute value is differentiated as the reference's ForwardDiff does: away
// from the kink, sign(1 - F).
//     value     w Q |1 - F|
//     gradient  -s w Q (c + 2 sum_r (A_r' x) A_r)
//     Hessian   -s w Q (2 sum_r A_r A_r') =: -s w Q T      -- T (lower triangle) is formed ONCE per goal (pcl_gram_kernel); a Hessian
//               evaluation is one scaled copy of it per term, plus the regularisers' diagonal, (dt, v) and (dt, dt) entries.
#pragma once

struct PclForm {
    const double *A;  // R x L, row-major
    const double *c;  // L or NULL
    int R, L, scope;  // scope 0: per member (L = x_dim), 1: joint (L = batch x_dim)
};

// element e of term t's argument: the address inside Z
__device__ __forceinline__ long long pcl_form_index(const PclForm &f, int t, int e, const int *__restrict__ x_offs, int x_dim, int N, int z_dim,
                                                    long long z_batch_stride) {
    const int mem = f.scope ? e / x_dim : t, r = f.scope ? e - mem * x_dim : e;
    // MEMBERS: one buffer, member offsets; TRAJ: buffer per seed, one offset
    return (z_batch_stride ? (long long)mem * z_batch_stride + x_offs[0] : (long long)x_offs[mem]) + (long long)(N - 1) * z_dim + r;
}

// value (member[t]), gradient (added to grad at the terminal knot) and the Hessian's coefficient -s w Q sigma (coef[t]) of every term
__global__ __launch_bounds__(256) void pcl_form_kernel(const double *__restrict__ Z, const PclForm f, const int *__restrict__ x_offs, const double *__restrict__ weights,
                                                       double Q, double sigma, int x_dim, int N, int z_dim, long long z_batch_stride, long long grad_batch_stride,
                                                       double *__restrict__ member, double *__restrict__ grad, double *__restrict__ coef) {
    extern __shared__ double lds[];  // p_r (R), then the reduction scratch
    __shared__ double red[8];
    const int t = blockIdx.x, tid = threadIdx.x;
    const double w = f.scope ? 1.0 : (weights ? weights[t] : 1.0);
    double lin = 0.0;
    if (f.c) {
        for (int e = tid; e < f.L; e += 256) lin += f.c[e] * Z[pcl_form_index(f, t, e, x_offs, x_dim, N, z_dim, z_batch_stride)];
    }
    lin = block_sum_256(lin, red);
    double F = lin;
    for (int r = 0; r < f.R; ++r) {
        const double *a = f.A + (long long)r * f.L;
        double s = 0.0;
        for (int e = tid; e < f.L; e += 256) s += a[e] * Z[pcl_form_index(f, t, e, x_offs, x_dim, N, z_dim, z_batch_stride)];
        s = block_sum_256(s, red);
        if (tid == 0) lds[r] = s;
        F += s * s;
    }
    __syncthreads();
    const double sgn = (1.0 - F) >= 0.0 ? 1.0 : -1.0;
    if (tid == 0) {
        if (member) member[t] = w * Q * fabs(1.0 - F);
        if (coef) coef[t] = -sgn * w * Q * sigma;
    }
    if (grad) {
        for (int e = tid; e < f.L; e += 256) {
            double g = f.c ? f.c[e] : 0.0;
            for (int r = 0; r < f.R; ++r) g += 2.0 * lds[r] * f.A[(long long)r * f.L + e];
            const int mem = f.scope ? e / x_dim : t;
            const long long zi = pcl_form_index(f, t, e, x_offs, x_dim, N, z_dim, z_batch_stride) - (z_batch_stride ? (long long)mem * z_batch_stride : 0);
            grad[(z_batch_stride ? (long long)mem * grad_batch_stride : 0) + zi] += -sgn * w * Q * g;
        }
    }
}

// T[i (i + 1) / 2 + j] = 2 sum_r A[r][i] A[r][j],  j <= i   (once per goal)
__global__ __launch_bounds__(256) void pcl_gram_kernel(const PclForm f, double *__restrict__ T) {
    const long long nT = (long long)f.L * (f.L + 1) / 2;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nT; e += (long long)gridDim.x * 256) {
        long long i = (long long)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
        while (i * (i + 1) / 2 > e) --i;
        while ((i + 1) * (i + 2) / 2 <= e) ++i;
        const long long j = e - i * (i + 1) / 2;
        double s = 0.0;
        for (int r = 0; r < f.R; ++r) s += f.A[(long long)r * f.L + i] * f.A[(long long)r * f.L + j];
        T[e] = 2.0 * s;
    }
}
// out[t nT + e] = coef[t] T[e]
__global__ __launch_bounds__(256) void pcl_scale_kernel(const double *__restrict__ T, const double *__restrict__ coef, long long nT, int n_terms, double *__restrict__ out) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nT * n_terms; e += (long long)gridDim.x * 256) out[e] = coef[e / nT] * T[e % nT];
}

// the regularisers' second derivatives, knot k of buffer tb: per regulariser [d2/dv_i^2 (dim) | d2/ddt dv_i (dim; dt_power >= 1) | d2/ddt^2 (1; dt_power 2)]
// J_r = 1/2 sum_k dt_k^p sum_i R_i v_{k,i}^2
__global__ __launch_bounds__(256) void pcl_reg_hess_kernel(const double *__restrict__ Z, const PclReg *__restrict__ regs, int n_regs, const double *__restrict__ Rv,
                                                           double sigma, int N, int z_dim, int dt_off, long long z_batch_stride, long long per_knot,
                                                           double *__restrict__ out) {
    __shared__ double red[8];
    const int k = blockIdx.x, tb = blockIdx.y, tid = threadIdx.x;
    const double *z = Z + (long long)tb * z_batch_stride + (long long)k * z_dim;
    double *o = out + ((long long)tb * N + k) * per_knot;
    const double h = z[dt_off];
    for (int r = 0; r < n_regs; ++r) {
        const PclReg R = regs[r];
        const double wv = R.pw == 0 ? 1.0 : (R.pw == 1 ? h : h * h);
        double s = 0.0;
        for (int i = tid; i < R.dim; i += 256) {
            const double v = z[R.off + i], ri = Rv[R.r0 + i];
            o[i] = sigma * wv * ri;
            // v_i is dt itself: the mixed entry lies on (dt, dt), where both orders of the partial meet
            if (R.pw >= 1) o[R.dim + i] = sigma * (R.pw == 1 ? 1.0 : 2.0 * h) * ri * v * (R.off + i == dt_off ? 2.0 : 1.0);
            s += ri * v * v;
        }
        if (R.pw == 2) {
            s = block_sum_256(s, red);
            if (tid == 0) o[2 * R.dim] = sigma * s;
        }
        o += R.dim * (R.pw >= 1 ? 2 : 1) + (R.pw == 2 ? 1 : 0);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// Objective of a variational context (option var_full): the knot holds the state x_0 and its sensitivities x_1 .. x_v, and
//     J = Q w_0 |1 - F(x_0,N)|  +  sum_i w_i (|x_i,N|^2)^2 / d^2  +  regularisers
// The middle term is the reference's UnitarySensitivityObjective (objectives.jl:437-453: scale^4 abs2(tr(U'U)) / n^2, tr(U'U) = |x|^2 of the
// iso-vec, n = d; Qs and scale^4 folded into w_i) at the terminal knot:
//     gradient  4 w_i |x|^2 x / d^2          Hessian  w_i (4 |x|^2 I + 8 x x') / d^2
// ONE launch (pcl_var_objective_kernel): workgroup k < N - 1 is the regulariser row of knot k; the last workgroup is the terminal knot -- its
// regulariser row first, then the terminal terms ADDED to the same gradient row, in component order (so a regulariser may cover any component
// of the knot) -- and the workgroup that arrives last at the ticket forms the sum in the fixed order of pcl_objective_sum_kernel.
// mode 1 (one workgroup): only the Hessian's coefficients, coef[0] = -s w_0 Q sigma, coef[i] = |x_i,N|^2 -- formed ONCE, not per entry.
// ------------------------------------------------------------------------------------------------------------------------------------------
#define PCL_VAROBJ_MAXC 3  // components of a variational knot (1 + v, v <= 2)
struct PclVarObj {
    const double *Z;
    double *grad, *value;  // grad may be null
    const PclReg *regs;
    const double *Rv;
    double *regval, *member;  // [N] regulariser values, [1 + v] terminal terms
    unsigned int *ticket;
    double *coef;  // mode 1
    PclForm f;     // the loss of component 0 (A and c null: no goal), L = x_dim of one component
    double w[PCL_VAROBJ_MAXC];
    int xo[PCL_VAROBJ_MAXC];
    int n_regs, v, d, N, z_dim, dt_off, mode;
    double Q, sigma;
};

__global__ __launch_bounds__(256) void pcl_var_objective_kernel(const PclVarObj a) {
    extern __shared__ double lds[];  // p_r (R)
    __shared__ double red[8];
    const int tid = threadIdx.x, L = a.f.L;
    const PclObjSum fin{a.value, a.regval, a.ticket, 1 + a.v, a.N, 0, a.N};
    if (a.mode == 0) {
        if ((int)blockIdx.x < a.N - 1) {
            pcl_regularizer_body((int)blockIdx.x, 0, a.Z, a.regs, a.n_regs, a.Rv, a.grad, a.regval, a.N, a.z_dim, a.dt_off, 0LL, fin, a.member);
            return;
        }
        pcl_regularizer_body(a.N - 1, 0, a.Z, a.regs, a.n_regs, a.Rv, a.grad, a.regval, a.N, a.z_dim, a.dt_off, 0LL, PclObjSum{}, nullptr);
        __syncthreads();  // the terminal knot's gradient row is complete: the terms below add to it
    }
    const double *zN = a.Z + (long long)(a.N - 1) * a.z_dim;
    double *gN = a.grad ? a.grad + (long long)(a.N - 1) * a.z_dim : nullptr;
    double t0 = 0.0, c0 = 0.0;
    if (a.f.A || a.f.c) {
        const double *x = zN + a.xo[0];
        double lin = 0.0;
        if (a.f.c)
            for (int e = tid; e < L; e += 256) lin += a.f.c[e] * x[e];
        lin = block_sum_256(lin, red);
        double F = lin;
        for (int r = 0; r < a.f.R; ++r) {
            const double *row = a.f.A + (long long)r * L;
            double s = 0.0;
            for (int e = tid; e < L; e += 256) s += row[e] * x[e];
            s = block_sum_256(s, red);
            if (tid == 0) lds[r] = s;
            F += s * s;
        }
        __syncthreads();
        const double sgn = (1.0 - F) >= 0.0 ? 1.0 : -1.0;
        t0 = a.w[0] * a.Q * fabs(1.0 - F);
        c0 = -sgn * a.w[0] * a.Q;
        if (gN && a.mode == 0)
            for (int e = tid; e < L; e += 256) {
                double g = a.f.c ? a.f.c[e] : 0.0;
                for (int r = 0; r < a.f.R; ++r) g += 2.0 * lds[r] * a.f.A[(long long)r * L + e];
                gN[a.xo[0] + e] += c0 * g;
            }
    }
    if (tid == 0) {
        if (a.mode == 0)
            __hip_atomic_store(a.member, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else
            a.coef[0] = c0 * a.sigma;
    }
    const double dd = (double)a.d * (double)a.d;
    for (int i = 1; i <= a.v; ++i) {
        double s = 0.0, term = 0.0;
        if (a.w[i] != 0.0) {  // (uniform)
            const double *x = zN + a.xo[i];
            for (int e = tid; e < L; e += 256) s += x[e] * x[e];
            s = block_sum_256(s, red);
            term = a.w[i] * (s * s) / dd;
            if (gN && a.mode == 0) {
                const double c = 4.0 * a.w[i] * s / dd;
                for (int e = tid; e < L; e += 256) gN[a.xo[i] + e] += c * x[e];
            }
        }
        if (tid == 0) {
            if (a.mode == 0)
                __hip_atomic_store(a.member + i, term, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                a.coef[i] = s;
        }
    }
    if (a.mode == 0) objective_finish(fin, a.member, red, false);
}

// The sensitivity term's Hessian: out[i (i + 1) / 2 + j] = c (4 s [i == j] + 8 x_i x_j), j <= i, c = sigma w / d^2, s = |x|^2 read from *s_ptr.
// A pure store stream (1.06 M doubles at d = 27): x is staged in LDS once, and every thread stores 16 bytes per step, a wave 1 KiB contiguous;
// one leading entry is peeled where `out` is not 16-byte aligned.
__device__ __forceinline__ void pcl_tri_decode(long long e, int &i, int &j) {
    long long r = (long long)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > e) --r;
    while ((r + 1) * (r + 2) / 2 <= e) ++r;
    i = (int)r;
    j = (int)(e - r * (r + 1) / 2);
}
__global__ __launch_bounds__(256) void pcl_sens_hess_kernel(const double *__restrict__ x, const double *__restrict__ s_ptr, double c, int L, double *__restrict__ out) {
    extern __shared__ double xs[];  // L
    for (int e = threadIdx.x; e < L; e += 256) xs[e] = x[e];
    __syncthreads();
    const double c4 = 4.0 * c * s_ptr[0], c8 = 8.0 * c;
    const long long nT = (long long)L * (L + 1) / 2;
    const long long head = (reinterpret_cast<unsigned long long>(out) & 15) ? 1 : 0;
    const long long npair = (nT - head) / 2;
    auto entry = [&](int i, int j) { return c8 * xs[i] * xs[j] + (i == j ? c4 : 0.0); };
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (head) out[0] = entry(0, 0);
        if ((nT - head) & 1) out[nT - 1] = entry(L - 1, L - 1);
    }
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npair; p += (long long)gridDim.x * 256) {
        const long long e = head + 2 * p;
        int i, j;
        pcl_tri_decode(e, i, j);
        const double v0 = entry(i, j);
        if (j == i) ++i, j = 0; else ++j;
        const double v1 = entry(i, j);
        *reinterpret_cast<double2_t *>(out + e) = double2_t{v0, v1};
    }
}

// Where a regulariser covers entries of a component that has a dense triangle (terminal knot only), its diagonal second derivatives belong to
// positions the triangle already holds.  Each position is emitted once: the triangle takes them,
//     out[i (i + 1) / 2 + i] += sigma (d[0][i] + h d[1][i] + h^2 d[2][i])      (d[p]: the summed R of the covering regularisers of dt_power p)
// and the terminal knot's regulariser block is written without them (pcl_gather_kernel picks the kept slots of the full block).
__global__ __launch_bounds__(256) void pcl_tri_diag_add_kernel(double *__restrict__ out, const double *__restrict__ d, const double *__restrict__ h_ptr, double sigma, int L) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= L) return;
    const double h = h_ptr[0];
    out[(long long)i * (i + 1) / 2 + i] += sigma * (d[i] + h * d[L + i] + h * h * d[2 * L + i]);
}
__global__ __launch_bounds__(256) void pcl_gather_kernel(const double *__restrict__ src, const int *__restrict__ idx, int count, double *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = src[idx[i]];
}

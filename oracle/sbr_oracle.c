/*
 * sbr_oracle.c — CPU restatement of the reference's hot path.
 *
 * *** TEST INFRASTRUCTURE ONLY. ***  Only tests/, __graft_entry__.smoke() and
 * bench.py's cpu_baseline leg may load this library.  The product path
 * (libsbr.so + HIP kernels) never links, loads or calls it.
 *
 * What it restates (file:line are into the Julia reference):
 *   learning   src/baseline/learning.jl:41-54 (solve_SIhomogeneous),
 *              :161-173 (compute_pdf_symbolic_baseline)
 *   ODE solver OrdinaryDiffEq 6.102.1 AutoTsit5(Rosenbrock23()) (Manifest.toml
 *              :1493-1497, Tsit5 1.5.0 :1679-1683, Rosenbrock 1.18.1
 *              :1643-1647) — NOT vendored in the reference; restated from the
 *              published methods: Tsit5 (Tsitouras 2011 tableau), Rosenbrock23
 *              (W-method, generic_lufact!/getrs, its error estimate and dense
 *              output), AutoSwitch's switch / switch-back (maxstiffstep 10,
 *              maxnonstiffstep 3, tolerances 9/10, dtfac 2), the PI controller
 *              (beta1=7/50, beta2=2/25, qmin=1/5, qmax=10, gamma=9/10,
 *              qoldinit=1e-4) with FastPower 1.1.3 fastpower (Manifest.toml
 *              :675-678), the Hairer-style initial dt and save_everystep
 *              knot semantics.  SBR_STIFF_SWITCH reports that the stiff
 *              branch ran (handled).
 *   hazard     src/baseline/solver.jl:153-185
 *   buffers    src/baseline/solver.jl:211-264
 *   bisection  src/baseline/solver.jl:308-376
 *   equilibrium src/baseline/solver.jl:413-462 (+ SolvedModel :79-95)
 *   AW path    src/baseline/solver.jl:495-532, AW_max :565
 *   sweeps     scripts/1_baseline.jl:151-192 (Fig 4), :224-267 (Fig 5),
 *              early-exit rule :236-244
 *   hetero     src/extensions/heterogeneity/heterogeneity_learning.jl:49-134,
 *              heterogeneity_solver.jl:48-144,175-210,241-293,316-375
 *   social     src/extensions/social_learning/social_learning_dynamics.jl:58-114,
 *              social_learning_solver.jl:63-263
 *   interest   src/extensions/interest_rates/value_function_solver.jl:66-112,
 *              interest_rate_solver.jl:51-150 (+ Tsit5's dense-output
 *              interpolant for `saveat`, OrdinaryDiffEqTsit5 — not vendored)
 *
 * Parity pinning: the reference is Julia and cannot run in this container or
 * on the GPU box.  This restatement is pinned by the
 * known answers extracted from the reference's committed figures
 * (tests/golden/, made by tools/extract_golden.py): Fig 3 ξ / τ_IN / AW
 * curves, the exact Fig 4 run boundary (2718 points), the exact Fig 5 run
 * masks at 500² and 5000², the social-learning figure.  Arithmetic below the
 * figure precision (~1e-5) — knot positions, ulp-level rounding — is
 * "parity unpinned" against Julia; the GPU engine is required to match this
 * file bit for bit.
 *
 * Arithmetic contract shared with the HIP kernels: IEEE binary64, compiled
 * with -ffp-contract=off; fma() appears exactly where OrdinaryDiffEq's
 * @muladd would put a muladd; exp/log/pow come from include/sbr_detmath.h.
 */
#include <math.h>

/* ode_determine_initdt's exponent 1/(order + 1): 6 (Tsit5's order 5, the restatement's
 * choice) unless a test sets another denominator to measure the choice (DESIGN.md §2,
 * tools/initdt_evidence.py) */
static double g_initdt_den = 6.0;
static int g_initdt_form = 0; /* 0: (0.01/md)^(1/den); 1: 10^(-(2 + log10(md))/den), initdt.jl's form */
void sbro_set_initdt_den(int d) { g_initdt_den = d > 0 ? (double)d : 6.0; }
static int g_initdt_ulps = 0; /* sensitivity probe: dt₁ moved by this many ulps */
void sbro_set_initdt(int form, int d) { g_initdt_form = form; g_initdt_den = d > 0 ? (double)d : 6.0; }
void sbro_set_initdt_ulps(int k) { g_initdt_ulps = k; }
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <stdio.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "../include/sbr_detmath.h"
#include "../include/sbr_status.h"

/* ------------------------------------------------------------------------ */
/* Tsit5 tableau (Tsitouras 2011), as in OrdinaryDiffEqTsit5's constant cache */
/* ------------------------------------------------------------------------ */
static const double C1 = 0.161, C2 = 0.327, C3 = 0.9, C4 = 0.9800255409045097;
static const double A21 = 0.161;
static const double A31 = -0.008480655492356989, A32 = 0.335480655492357;
static const double A41 = 2.897153057105493, A42 = -6.359448489975075, A43 = 4.3622954328695815;
static const double A51 = 5.325864828439257, A52 = -11.748883564062828, A53 = 7.4955393428898365,
                    A54 = -0.09249506636175525;
static const double A61 = 5.86145544294642, A62 = -12.92096931784711, A63 = 8.159367898576159,
                    A64 = -0.071584973281401, A65 = -0.028269050394068383;
static const double A71 = 0.09646076681806523, A72 = 0.01, A73 = 0.4798896504144996,
                    A74 = 1.379008574103742, A75 = -3.290069515436081, A76 = 2.324710524099774;
static const double BT1 = -0.00178001105222577714, BT2 = -0.0008164344596567469,
                    BT3 = 0.007880878010261995, BT4 = -0.1447110071732629,
                    BT5 = 0.5823571654525552, BT6 = -0.45808210592918697,
                    BT7 = 0.015151515151515152;
/* alg_stability_size(::Tsit5) (OrdinaryDiffEqTsit5 alg_utils) */
#ifndef SBRO_TSIT5_STABILITY
#define SBRO_TSIT5_STABILITY 3.5068
#endif
static const double TSIT5_STABILITY = SBRO_TSIT5_STABILITY;

/* Rosenbrock23Tableau (OrdinaryDiffEqRosenbrock 1.18.1): c32 = 6 + sqrt(2), d = 1/(2 + sqrt(2)) */
static const double ROS23_C32 = 0x1.da827999fcef3p+2; /* 7.414213562373095 */
static const double ROS23_D = 0x1.2bec333018867p-2;   /* 0.2928932188134525 */

/* OrdinaryDiffEq PI-controller defaults.  The composite algorithm takes the
 * betas of its current (first) algorithm at init (_composite_beta1_default):
 * Tsit5's 7/50, 2/25, held for the whole solve — reset_alg_dependent_opts!
 * compares the Float64 opts with the Rational defaults (7//50 ≠ 0.14 exactly),
 * so a switch to Rosenbrock23 does not replace them; qmin = max, qmax = min
 * over the two algorithms' defaults (1/5, 10), gamma 9/10. */
#define CTL_BETA1 0.14   /* 7//50 */
#define CTL_BETA2 0.08   /* 2//25 */
#define CTL_INV_QMIN 5.0 /* qmin = 1//5 */
#define CTL_INV_QMAX 0.1 /* qmax = 10 */
#define CTL_GAMMA 0.9
#define CTL_QOLDMIN 1e-4
/* AutoSwitch defaults (OrdinaryDiffEqCore composite_algs): maxstiffstep 10,
 * maxnonstiffstep 3, nonstifftol = stifftol = 9/10, dtfac 2 */
#define AUTOSWITCH_TOL 0.9
#define AUTOSWITCH_MAXSTIFF 10
#define AUTOSWITCH_MAXNONSTIFF 3
#define AUTOSWITCH_DTFAC 2.0

static inline double dmin(double a, double b) { return a < b ? a : b; }
static inline double dmax(double a, double b) { return a > b ? a : b; }

/* ------------------------------------------------------------------------ */
/* growable knot arrays                                                      */
/* ------------------------------------------------------------------------ */
typedef struct {
    double* t;
    double* x; /* n * K values, row-major [knot][group] */
    int64_t n, cap;
    int K;
} knots_t;

static int knots_push(knots_t* kn, double t, const double* x)
{
    if (kn->n == kn->cap) {
        int64_t nc = kn->cap ? kn->cap * 2 : 1024;
        double* nt = (double*)realloc(kn->t, (size_t)nc * sizeof(double));
        if (!nt) return -1;
        kn->t = nt;
        double* nx = (double*)realloc(kn->x, (size_t)nc * kn->K * sizeof(double));
        if (!nx) return -1;
        kn->x = nx;
        kn->cap = nc;
    }
    kn->t[kn->n] = t;
    memcpy(kn->x + kn->n * kn->K, x, (size_t)kn->K * sizeof(double));
    kn->n++;
    return 0;
}

static void knots_free(knots_t* kn)
{
    free(kn->t);
    free(kn->x);
    memset(kn, 0, sizeof(*kn));
}

/* ------------------------------------------------------------------------ */
/* Interpolations.jl 0.15.1 gridded Linear, Throw() extrapolation            */
/* ------------------------------------------------------------------------ */
/* searchsortedlast over t[0..n): count of elements <= x, minus 1 (−1 if none) */
static inline int64_t ssl(const double* t, int64_t n, double x)
{
    int64_t lo = 0, hi = n; /* first index with t > x */
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if (t[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

/* value at x of the piecewise-linear interpolant through (t[i], v[i*stride]).
 * Out of [t0, t_{n-1}] (or NaN) -> sets *oob and returns NaN (BoundsError). */
static inline double interp_s(const double* t, const double* v, int64_t stride, int64_t n, double x,
                              int* oob)
{
    if (n < 2 || !(x >= t[0] && x <= t[n - 1])) { /* (a 1-knot grid has no interpolant) */
        *oob = 1;
        return NAN;
    }
    int64_t j = ssl(t, n, x);
    if (j > n - 2) j = n - 2;
    if (j < 0) j = 0;
    double d = (x - t[j]) / (t[j + 1] - t[j]);
    return v[j * stride] * (1.0 - d) + v[(j + 1) * stride] * d;
}
#define INTERP(t, v, n, x, oob) interp_s((t), (v), 1, (n), (x), (oob))

/* ForwardDiff derivative of the same interpolant at x (a Dual in the time
 * argument): δ = (x − t_j)/Δ carries partial 1/Δ, so the value's partial is
 * v_j·(−(1/Δ)) + v_{j+1}·(1/Δ).  Used for Rosenbrock23's ∂f/∂t. */
static inline double interp_dx(const double* t, const double* v, int64_t stride, int64_t n, double x, int* oob)
{
    if (n < 2 || !(x >= t[0] && x <= t[n - 1])) { *oob = 1; return NAN; }
    int64_t j = ssl(t, n, x);
    if (j > n - 2) j = n - 2;
    if (j < 0) j = 0;
    const double r = 1.0 / (t[j + 1] - t[j]);
    return v[j * stride] * (-r) + v[(j + 1) * stride] * r;
}

/* ------------------------------------------------------------------------ */
/* The ODE solver: OrdinaryDiffEq's AutoTsit5(Rosenbrock23()) at the         */
/* reference's reltol = abstol = eps() (learning.jl:51,                      */
/* heterogeneity_learning.jl:74, social_learning_dynamics.jl:71,             */
/* value_function_solver.jl:105).  Restated from OrdinaryDiffEqCore 1.34.0   */
/* (solve! / loopheader! / loopfooter!, PIController, AutoSwitch),           */
/* OrdinaryDiffEqTsit5 1.5.0 and OrdinaryDiffEqRosenbrock 1.18.1             */
/* (Manifest.toml:1511-1515, 1679-1683, 1643-1647) — not vendored.           */
/* Every solving entry point named *_opt (sweeps, points, hetero learning)   */
/* ends with the arguments rtol, atol, ode_maxiters: they hold for each ODE  */
/* solve of the call — the learning solve, the interest value function, the  */
/* social extension's initial solve and every forced iterate — like the      */
/* device's sbr_opts (include/sbr.h).  oracle.py defaults them to eps(),     */
/* eps() and SBR_DEFAULT_ODE_MAXITERS.  Arguments, not a global: the sweeps  */
/* are OpenMP-parallel and one loaded library serves a whole test session.   */
/* ------------------------------------------------------------------------ */
/* rhs(ctx, t, x[m], dx[m], &oob) */
typedef void (*rhs_fn)(void* ctx, double t, const double* x, double* dx, int* oob);
/* Jacobian J[m×m] (row-major, J[i*m+j] = ∂f_i/∂x_j) and ∂f/∂t at (t, x), as
 * ForwardDiff's dual arithmetic evaluates them through the RHS expression */
typedef void (*jac_fn)(void* ctx, double t, const double* x, double* J, double* dT, int* oob);

typedef struct {
    int64_t naccept, nreject;
    int64_t nstiff;  /* attempted Rosenbrock23 steps */
    int32_t nswitch; /* algorithm switches (either direction) */
    uint32_t status;
    double t_switch; /* time of the first switch to Rosenbrock23 (NaN if never) */
} ode_stats_t;

#define MAXK 64
#define MAXJ 16 /* largest system with a Rosenbrock23 branch (hetero K <= 8) */

/* RMS norm over m components (DiffEqBase ODE_DEFAULT_NORM); |x| when m == 1 */
static inline double rms_norm(const double* v, int m)
{
    if (m == 1) return fabs(v[0]);
    double s = 0.0;
    for (int i = 0; i < m; i++) s = s + v[i] * v[i];
    return sqrt(s / (double)m);
}

/* AutoSwitchCache: successive stiffness-test positives count up, negatives
 * down (composite_algs.jl); is_stiff: |eigen_est·dt / stability(Tsit5)| >
 * tol, tested in every loopheader! (after the accept/reject dt update,
 * before fix_dt_at_bounds!).  Returns 1 when the algorithm changes; the
 * switch scales dt by dtfac (×2 to Rosenbrock23, ÷2 back to Tsit5). */
typedef struct {
    int count;
    int stiff; /* current algorithm is Rosenbrock23 */
} autoswitch_t;

static inline int autoswitch_choose(autoswitch_t* as, double eigen_est, double* dt)
{
    double stiffness = fabs(eigen_est * *dt / TSIT5_STABILITY);
    int is_stiff = stiffness > AUTOSWITCH_TOL; /* NaN -> false */
    if (is_stiff) as->count = as->count < 0 ? 1 : as->count + 1;
    else as->count = as->count > 0 ? -1 : as->count - 1;
    if (!as->stiff && as->count > AUTOSWITCH_MAXSTIFF) {
        *dt = *dt * AUTOSWITCH_DTFAC;
        as->stiff = 1;
        return 1;
    }
    if (as->stiff && as->count < -AUTOSWITCH_MAXNONSTIFF) {
        *dt = *dt / AUTOSWITCH_DTFAC;
        as->stiff = 0;
        return 1;
    }
    return 0;
}

/* LinearAlgebra/LinearSolve generic_lufact! with RowMaximum pivoting (the
 * default LinearSolve choice for length(b) <= 10: GenericLUFactorization):
 * column scaling by the reciprocal pivot, rank-1 updates A[i,j] -= A[i,k]·A[k,j]
 * (no fma), row-major A[i*m+j]. */
static void lu_factor(double* A, int m, int* piv)
{
    for (int k = 0; k < m; k++) {
        int kp = k;
        if (k < m - 1) {
            double amax = fabs(A[k * m + k]);
            for (int i = k + 1; i < m; i++) {
                const double ai = fabs(A[i * m + k]);
                if (ai > amax) { kp = i; amax = ai; }
            }
        }
        piv[k] = kp;
        if (A[kp * m + k] != 0.0) {
            if (kp != k)
                for (int j = 0; j < m; j++) { double tmp = A[k * m + j]; A[k * m + j] = A[kp * m + j]; A[kp * m + j] = tmp; }
            const double inv = 1.0 / A[k * m + k];
            for (int i = k + 1; i < m; i++) A[i * m + k] = A[i * m + k] * inv;
        }
        for (int j = k + 1; j < m; j++)
            for (int i = k + 1; i < m; i++) A[i * m + j] = A[i * m + j] - A[i * m + k] * A[k * m + j];
    }
}

/* ldiv! on the factors = LAPACK getrs (laswp, unit-lower then upper trsv,
 * column-oriented axpy updates y += (−x_j)·a_ij in fma, division by the pivot) */
static void lu_solve(const double* A, const int* piv, int m, double* b)
{
    for (int k = 0; k < m; k++)
        if (piv[k] != k) { double tmp = b[k]; b[k] = b[piv[k]]; b[piv[k]] = tmp; }
    for (int j = 0; j < m; j++) {
        const double a = -b[j];
        for (int i = j + 1; i < m; i++) b[i] = fma(a, A[i * m + j], b[i]);
    }
    for (int j = m - 1; j >= 0; j--) {
        b[j] = b[j] / A[j * m + j];
        const double a = -b[j];
        for (int i = 0; i < j; i++) b[i] = fma(a, A[i * m + j], b[i]);
    }
}

/* opnorm(J, Inf): max row sum of |J_ij| (NaN-propagating max) — the
 * eigen_est calc_J! sets for a CompositeAlgorithm */
static double opnorm_inf(const double* J, int m)
{
    double nrm = 0.0;
    for (int i = 0; i < m; i++) {
        double s = 0.0;
        for (int j = 0; j < m; j++) s = s + fabs(J[i * m + j]);
        nrm = (nrm != nrm || s != s) ? NAN : (s > nrm ? s : nrm);
    }
    return nrm;
}

/* called after every accepted step with (tprev, t, dt, uprev, u, k) — the
 * integrator state OrdinaryDiffEq's savevalues! sees (saveat interpolation);
 * stiff = 1: k = {k1, k2} of Rosenbrock23, else k1..k7 of Tsit5 */
typedef void (*step_fn)(void* ctx, double tprev, double t, double dt, const double* uprev, const double* u,
                        const double* const* k, int stiff);

typedef struct {
    rhs_fn f;
    jac_fn jac; /* NULL: no Rosenbrock23 branch restated for this RHS (flag SBR_ODE_FAILED if needed) */
    void* ctx;
} ode_sys_t;

/* One Tsit5 step (perform_step!, Tsit5Cache, @muladd): u, k[0..6], EEst and
 * the AutoSwitch eigenvalue estimate |(k7 − k6)/(u − g6)|_∞ (Hairer II p. 22) */
static void tsit5_step(const ode_sys_t* S, int m, double t, double dt, const double* x, double* const* k,
                       double* u, double rtol, double atol, double* EEst, double* eig, int* oob)
{
    double tmp[MAXK], tmp6[MAXK], buf[MAXK];
    double *k1 = k[0], *k2 = k[1], *k3 = k[2], *k4 = k[3], *k5 = k[4], *k6 = k[5], *k7 = k[6];
    double a = dt * A21;
    for (int i = 0; i < m; i++) tmp[i] = fma(a, k1[i], x[i]);
    S->f(S->ctx, fma(C1, dt, t), tmp, k2, oob);
    for (int i = 0; i < m; i++) tmp[i] = fma(dt, fma(A31, k1[i], A32 * k2[i]), x[i]);
    S->f(S->ctx, fma(C2, dt, t), tmp, k3, oob);
    for (int i = 0; i < m; i++) tmp[i] = fma(dt, fma(A41, k1[i], fma(A42, k2[i], A43 * k3[i])), x[i]);
    S->f(S->ctx, fma(C3, dt, t), tmp, k4, oob);
    for (int i = 0; i < m; i++)
        tmp[i] = fma(dt, fma(A51, k1[i], fma(A52, k2[i], fma(A53, k3[i], A54 * k4[i]))), x[i]);
    S->f(S->ctx, fma(C4, dt, t), tmp, k5, oob);
    for (int i = 0; i < m; i++)
        tmp6[i] = fma(dt, fma(A61, k1[i], fma(A62, k2[i], fma(A63, k3[i], fma(A64, k4[i], A65 * k5[i])))), x[i]);
    S->f(S->ctx, t + dt, tmp6, k6, oob);
    for (int i = 0; i < m; i++)
        u[i] = fma(dt, fma(A71, k1[i], fma(A72, k2[i], fma(A73, k3[i], fma(A74, k4[i], fma(A75, k5[i], A76 * k6[i]))))),
                   x[i]);
    S->f(S->ctx, t + dt, u, k7, oob);
    double e = 0.0;
    int e_nan = 0;
    for (int i = 0; i < m; i++) {
        double r = fabs((k7[i] - k6[i]) / (u[i] - tmp6[i]));
        if (r != r) e_nan = 1;
        else if (r > e) e = r;
    }
    *eig = e_nan ? NAN : e;
    for (int i = 0; i < m; i++) {
        double ut = dt * fma(BT1, k1[i],
                             fma(BT2, k2[i], fma(BT3, k3[i], fma(BT4, k4[i], fma(BT5, k5[i], fma(BT6, k6[i], BT7 * k7[i]))))));
        buf[i] = ut / fma(dmax(fabs(x[i]), fabs(u[i])), rtol, atol);
    }
    *EEst = rms_norm(buf, m);
}

/* One Rosenbrock23 step (perform_step!, Rosenbrock23Cache, @muladd), with
 * W = J − I/(dt·d) (calc_W!, W_transform) factored once and the stages
 * k = (W \ b)·(−1/(dt·d)); FSAL fsal = f(uprev, t); eigen_est = ‖J‖_∞. */
static void ros23_step(const ode_sys_t* S, int m, double t, double dt, const double* x, const double* fsal,
                       double* u, double* fnew, double* k1, double* k2, double rtol, double atol, double* EEst,
                       double* eig, int* oob)
{
    double J[MAXJ * MAXJ], W[MAXJ * MAXJ], dT[MAXJ], b[MAXJ], f1[MAXJ], k3[MAXJ], tmp[MAXJ], buf[MAXJ];
    int piv[MAXJ];
    const double dtg = dt * ROS23_D;
    const double invdtg = 1.0 / dtg, neginvdtg = -(1.0 / dtg);
    const double dto2 = dt / 2.0, dto6 = dt / 6.0;
    S->jac(S->ctx, t, x, J, dT, oob);
    *eig = opnorm_inf(J, m);
    for (int i = 0; i < m * m; i++) W[i] = J[i];
    for (int i = 0; i < m; i++) W[i * m + i] = fma(-1.0, invdtg, J[i * m + i]);
    lu_factor(W, m, piv);
    for (int i = 0; i < m; i++) b[i] = fsal[i] + dtg * dT[i]; /* calc_tderivative!: linsolve_tmp */
    lu_solve(W, piv, m, b);
    for (int i = 0; i < m; i++) k1[i] = b[i] * neginvdtg;
    for (int i = 0; i < m; i++) tmp[i] = fma(dto2, k1[i], x[i]);
    S->f(S->ctx, t + dto2, tmp, f1, oob);
    for (int i = 0; i < m; i++) b[i] = f1[i] - k1[i];
    lu_solve(W, piv, m, b);
    for (int i = 0; i < m; i++) k2[i] = fma(b[i], neginvdtg, k1[i]);
    for (int i = 0; i < m; i++) u[i] = fma(dt, k2[i], x[i]);
    S->f(S->ctx, t + dt, u, fnew, oob);
    for (int i = 0; i < m; i++)
        b[i] = fma(dt, dT[i], fma(-2.0, k1[i] - fsal[i], fma(-ROS23_C32, k2[i] - f1[i], fnew[i])));
    lu_solve(W, piv, m, b);
    for (int i = 0; i < m; i++) k3[i] = b[i] * neginvdtg;
    for (int i = 0; i < m; i++) {
        const double ut = dto6 * (fma(-2.0, k2[i], k1[i]) + k3[i]);
        buf[i] = ut / fma(dmax(fabs(x[i]), fabs(u[i])), rtol, atol);
    }
    *EEst = rms_norm(buf, m);
}

/* kn == NULL: no knots kept (saveat problems keep only what on_step saves) */
static int ode_solve_cb(const ode_sys_t* S, int m, double t0, double t1, const double* x0, double rtol, double atol,
                        int64_t maxiters, knots_t* kn, ode_stats_t* st, step_fn on_step, void* step_ctx)
{
    double x[MAXK], kk[7][MAXK], u[MAXK], sk[MAXK], buf[MAXK], f1[MAXK], fnew[MAXK];
    double* const k[7] = {kk[0], kk[1], kk[2], kk[3], kk[4], kk[5], kk[6]};
    double* fsal = kk[0]; /* k1 of Tsit5 = fsalfirst */
    int oob = 0;
    memset(st, 0, sizeof(*st));
    if (kn) kn->K = m;
    const double dtmax = t1 - t0;
    const double dtmin = sbr_jl_eps(dmax(fabs(t0), fabs(t1)));

    /* ---- ode_determine_initdt (OrdinaryDiffEqCore initdt.jl, @muladd) ---- */
    for (int i = 0; i < m; i++) { x[i] = x0[i]; sk[i] = fma(fabs(x0[i]), rtol, atol); }
    for (int i = 0; i < m; i++) buf[i] = x0[i] / sk[i];
    double d0 = rms_norm(buf, m);
    S->f(S->ctx, t0, x, fsal, &oob);
    for (int i = 0; i < m; i++) buf[i] = fsal[i] / sk[i];
    double d1 = rms_norm(buf, m);
    double dt0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : (d0 / d1) / 100.0;
    dt0 = dmin(dt0, dtmax);
    double dt;
    if (dt0 < 10.0 * 2.220446049250313e-16) {
        dt = dmax(1e-6, dtmin);
    } else {
        for (int i = 0; i < m; i++) u[i] = fma(dt0, fsal[i], x0[i]);
        S->f(S->ctx, t0 + dt0, u, f1, &oob);
        int same = 1;
        for (int i = 0; i < m; i++) same &= (fsal[i] == f1[i]);
        if (same) {
            dt = dmax(dtmin, 100.0 * dt0);
        } else {
            for (int i = 0; i < m; i++) buf[i] = (f1[i] - fsal[i]) / sk[i];
            double d2 = rms_norm(buf, m) / dt0;
            double md = dmax(d1, d2);
            /* dt₁ = (0.01/max(d₁, d₂))^(1/6).  initdt.jl's own expression is recalled as
             * 10^(-(2 + log10(md)) / get_current_alg_order) with Tsit5's order 5, i.e. 1/5;
             * the figures cannot separate the two except at one knife-edge cell, (β₂₈₄,
             * u₉₅) of the 500² mask (no run in the figure): 1/6 gives no run for every
             * first step within ±4 ulps, 1/5 for 4-5 of 9 (tools/initdt_evidence.py →
             * profiles/r03_initdt_exponent.json).  Kept: 1/6. */
            double dt1 = (md <= 1e-15) ? dmax(1e-6, dt0 * 1e-3)
                         : (g_initdt_form ? sbr_exp10(-(2.0 + sbr_log10(md)) / g_initdt_den)
                                          : sbr_pow_pos(0.01 / md, 1.0 / g_initdt_den));
            for (int k = 0; k < g_initdt_ulps; k++) dt1 = nextafter(dt1, INFINITY);
            for (int k = 0; k > g_initdt_ulps; k--) dt1 = nextafter(dt1, -INFINITY);
            dt = dmax(dtmin, dmin(dmin(100.0 * dt0, dt1), dtmax));
        }
    }

    /* ---- main loop (solve! / loopheader! / perform_step! / loopfooter!) ---- */
    const double snap = 100.0 * sbr_jl_eps(t1);
    double t = t0, qold = CTL_QOLDMIN;
    double qold_b2 = sbr_fastpow(qold, CTL_BETA2); /* fastpower(qold, β2), refreshed when qold changes */
    double eig = 1.0;                              /* integrator.eigen_est = 1/oneunit(t) at init */
    autoswitch_t as = {0, 0};
    st->t_switch = NAN;
    if (kn && knots_push(kn, t0, x)) return -1;
    int64_t iter = 0;
    while (t < t1) {
        if (++iter > maxiters) { st->status |= SBR_ODE_MAXITERS; break; }
        /* choose_algorithm!: AutoSwitch on the current eigen_est and dt; the new
         * algorithm's initialize! re-evaluates fsalfirst = f(uprev, t) */
        if (autoswitch_choose(&as, eig, &dt)) {
            st->nswitch++;
            if (as.stiff && st->t_switch != st->t_switch) st->t_switch = t;
            if (as.stiff && !S->jac) { st->status |= SBR_ODE_FAILED; break; }
            S->f(S->ctx, t, x, fsal, &oob);
        }
        dt = dmin(dtmax, dt); /* fix_dt_at_bounds! */
        dt = dmax(dt, dtmin);
        dt = dmin(dt, t1 - t); /* modify_dt_for_tstops! */

        /* check_error!: dt forced to dtmin short of the end (ReturnCode.DtLessThanMin) */
        if (dt <= dtmin && t + dt < t1) { st->status |= SBR_ODE_FAILED; break; }
        double EEst;
        if (as.stiff) {
            st->nstiff++;
            ros23_step(S, m, t, dt, x, fsal, u, fnew, k[1], k[2], rtol, atol, &EEst, &eig, &oob);
        } else {
            tsit5_step(S, m, t, dt, x, k, u, rtol, atol, &EEst, &eig, &oob);
        }
        if (EEst != EEst) { st->status |= SBR_ODE_FAILED; break; } /* NaN trial state: Unstable */
        /* stepsize_controller!(PIController): q11 = fastpower(EEst, β1),
         * q = q11 / fastpower(qold, β2), clamped q/γ (FastPower 1.1.3) */
        double q, q11 = 0.0;
        if (EEst == 0.0) {
            q = CTL_INV_QMAX;
        } else {
#ifdef SBRO_DIAG_EXACTPOW
            q11 = sbr_exp(CTL_BETA1 * sbr_log(EEst));
            q = sbr_exp(CTL_BETA1 * sbr_log(EEst) - CTL_BETA2 * sbr_log(qold));
#else
            q11 = sbr_fastpow(EEst, CTL_BETA1);
            q = q11 / qold_b2;
#endif
            q = dmax(CTL_INV_QMAX, dmin(CTL_INV_QMIN, q / CTL_GAMMA));
        }
        if (EEst <= 1.0) { /* accept: step_accept_controller!, apply_step! */
            st->naccept++;
            double dtnew = dt / q;
            const double qn = dmax(EEst, CTL_QOLDMIN);
            if (qn != qold) { qold = qn; qold_b2 = sbr_fastpow(qold, CTL_BETA2); }
            double tn = t + dt;
            if (fabs(tn - t1) < snap) tn = t1; /* 100 eps(max(t, t_end)), t < t_end */
            if (on_step) {
                if (as.stiff) {
                    const double* const ks[2] = {k[1], k[2]};
                    on_step(step_ctx, t, tn, dt, x, u, ks, 1);
                } else {
                    const double* const ks[7] = {k[0], k[1], k[2], k[3], k[4], k[5], k[6]};
                    on_step(step_ctx, t, tn, dt, x, u, ks, 0);
                }
            }
            t = tn;
            const double* fl = as.stiff ? fnew : k[6]; /* fsallast */
            for (int i = 0; i < m; i++) { x[i] = u[i]; fsal[i] = fl[i]; }
            dt = dmax(dmin(dtmax, dtnew), dtmin); /* calc_dt_propose! */
            if (kn && knots_push(kn, t, x)) return -1;
        } else { /* reject: step_reject_controller!, dt /= min(1/qmin, q11/γ) */
            st->nreject++;
            dt = dt / dmin(CTL_INV_QMIN, q11 / CTL_GAMMA);
        }
        if (!(dt > 0.0) || !isfinite(dt)) { st->status |= SBR_ODE_FAILED; break; }
    }
    if (st->nswitch > 0) st->status |= SBR_STIFF_SWITCH;
    if (oob) st->status |= SBR_OOB;
    return 0;
}

static int ode_solve(const ode_sys_t* S, int m, double t0, double t1, const double* x0, double rtol, double atol,
                     int64_t maxiters, knots_t* kn, ode_stats_t* st)
{
    return ode_solve_cb(S, m, t0, t1, x0, rtol, atol, maxiters, kn, st, NULL, NULL);
}

/* ------------------------------------------------------------------------ */
/* Baseline learning: dx/dt = β x (1 − x)  (learning.jl:45-48)              */
/* ------------------------------------------------------------------------ */
static void rhs_logistic(void* ctx, double t, const double* x, double* dx, int* oob)
{
    (void)t; (void)oob;
    double beta = *(const double*)ctx;
    dx[0] = (beta * x[0]) * (1.0 - x[0]);
}

/* ForwardDiff through (β·x)·(1 − x): partials β and −1, product rule
 * β·(1 − x) + (−1)·(β·x); autonomous: ∂f/∂t = 0 */
static void jac_logistic(void* ctx, double t, const double* x, double* J, double* dT, int* oob)
{
    (void)t; (void)oob;
    double beta = *(const double*)ctx;
    J[0] = beta * (1.0 - x[0]) + (-1.0) * (beta * x[0]);
    dT[0] = 0.0;
}

static const ode_sys_t* sys_logistic(double* beta, ode_sys_t* S)
{
    S->f = rhs_logistic; S->jac = jac_logistic; S->ctx = beta;
    return S;
}

int64_t sbro_learn_logistic(double beta, double t0, double t1, double x0, double rtol, double atol,
                            int64_t maxiters, double* t_out, double* G_out, int64_t cap, int64_t* stats)
{
    knots_t kn = {0};
    ode_stats_t st;
    ode_sys_t S;
    if (ode_solve(sys_logistic(&beta, &S), 1, t0, t1, &x0, rtol, atol, maxiters, &kn, &st)) {
        knots_free(&kn);
        return -1;
    }
    int64_t n = kn.n;
    if (stats) {
        stats[0] = st.naccept; stats[1] = st.nreject; stats[2] = st.status; stats[3] = n;
        memcpy(&stats[4], &st.t_switch, 8); stats[5] = st.nswitch; stats[6] = st.nstiff;
    }
    if (n > cap) n = -n; /* caller buffer too small: return -needed */
    else {
        memcpy(t_out, kn.t, (size_t)kn.n * sizeof(double));
        memcpy(G_out, kn.x, (size_t)kn.n * sizeof(double));
    }
    knots_free(&kn);
    return n;
}

/* ------------------------------------------------------------------------ */
/* Hazard rate on the τ̄ grid (solver.jl:153-185)                           */
/* ------------------------------------------------------------------------ */
typedef struct {
    double* tau; /* N_eta knots: t_i <= eta, then eta appended if not last */
    double* hr;
    int64_t n;
    int oob;
} hazard_t;

static void hazard_free(hazard_t* h) { free(h->tau); free(h->hr); memset(h, 0, sizeof(*h)); }

/* pdf given at the ODE knots (g[i]); explicit_grid=1 reproduces the `grid=`
 * branch (solver.jl:163-164: always append η) used by the hetero solver. */
static int hazard_rate(const double* t, const double* g, int64_t n, double p, double a, double eta,
                       int explicit_grid, hazard_t* h)
{
    memset(h, 0, sizeof(*h));
    int64_t m = 0;
    while (m < n && t[m] <= eta) m++; /* knots are sorted: the .<= η mask is a prefix */
    int push = explicit_grid ? 1 : (m == 0 || t[m - 1] != eta);
    int64_t N = m + push;
    h->tau = (double*)malloc((size_t)(N > 0 ? N : 1) * sizeof(double));
    h->hr = (double*)malloc((size_t)(N > 0 ? N : 1) * sizeof(double));
    double* pdf = (double*)malloc((size_t)(N > 0 ? N : 1) * sizeof(double));
    double* I = (double*)malloc((size_t)(N > 0 ? N : 1) * sizeof(double));
    if (!h->tau || !h->hr || !pdf || !I) { free(pdf); free(I); return -1; }
    for (int64_t i = 0; i < m; i++) { h->tau[i] = t[i]; pdf[i] = g[i]; }
    if (push) {
        h->tau[m] = eta;
        pdf[m] = INTERP(t, g, n, eta, &h->oob);
    }
    h->n = N;
    /* cumulative trapezoid of eg(τ) = exp(aτ)·pdf(τ) (solver.jl:168-176) */
    I[0] = 0.0;
    double eprev = sbr_exp(a * h->tau[0]) * pdf[0];
    for (int64_t i = 1; i < N; i++) {
        double ei = sbr_exp(a * h->tau[i]) * pdf[i];
        I[i] = I[i - 1] + (0.5 * (eprev + ei)) * (h->tau[i] - h->tau[i - 1]);
        eprev = ei;
    }
    double Ieta = I[N - 1];
    double omp = 1.0 - p;
    for (int64_t i = 0; i < N; i++)
        h->hr[i] = ((p * sbr_exp(a * h->tau[i])) * pdf[i]) / ((p * I[i]) + (omp * Ieta));
    free(pdf);
    free(I);
    return 0;
}

/* ------------------------------------------------------------------------ */
/* optimal_buffer (solver.jl:211-264)                                       */
/* ------------------------------------------------------------------------ */
static void optimal_buffer(double u, const double* tau, const double* hr, int64_t n, double t_end,
                           double* tin_out, double* tout_out)
{
    int any = 0, all = 1;
    int64_t first_above = -1, last_above = -1;
    for (int64_t i = 0; i < n; i++) {
        int ab = hr[i] > u;
        any |= ab;
        all &= ab;
        if (ab) { if (first_above < 0) first_above = i; last_above = i; }
    }
    if (!any) { *tin_out = t_end; *tout_out = t_end; return; }
    if (all) { *tin_out = tau[0]; *tout_out = tau[n - 1]; return; }
    double tin = t_end, tout = t_end;
    for (int64_t i = 0; i + 1 < n; i++) {
        if (!(hr[i] > u) && (hr[i + 1] > u)) {
            tin = tau[i] + ((u - hr[i]) * (tau[i + 1] - tau[i])) / (hr[i + 1] - hr[i]);
            break;
        }
    }
    for (int64_t i = n - 2; i >= 0; i--) {
        if ((hr[i] > u) && !(hr[i + 1] > u)) {
            tout = tau[i] + ((u - hr[i]) * (tau[i + 1] - tau[i])) / (hr[i + 1] - hr[i]);
            break;
        }
    }
    if (tin == t_end) tin = tau[first_above];
    if (tout == t_end) tout = tau[last_above];
    *tin_out = tin;
    *tout_out = tout;
}

/* ------------------------------------------------------------------------ */
/* compute_ξ bisection (solver.jl:308-376)                                  */
/* returns status bits; *xi / *tol set; *iters = loop iterations executed   */
/* ------------------------------------------------------------------------ */
/* compute_ξ's ξ_guess (solver.jl:309-312; solve_equilibrium_baseline passes it through, :413,441):
 * NaN = the default midpoint.  Set by tests around single calls (sbro_set_xi_guess). */
static double g_xi_guess = NAN;
void sbro_set_xi_guess(double g) { g_xi_guess = g; }

static uint32_t compute_xi(double tin, double tout, const double* t, const double* G, int64_t n, double kappa,
                           int32_t max_iters, double* xi_out, double* tol_out, int32_t* iters)
{
    const double tolerance = 10.0 * sbr_jl_eps(kappa);
    double xnew = g_xi_guess == g_xi_guess ? g_xi_guess : (tin + tout) / 2.0, xmin = tin, xmax = tout;
    int oob = 0;
    *xi_out = NAN;
    *tol_out = INFINITY;
    for (int32_t iter = 1; iter <= max_iters; iter++) {
        *iters = iter;
        double d = xmin - xmax;
        if (fabs(d) < 2.0 * sbr_jl_eps(d)) return SBR_NO_RUN_COLLAPSE;
        if (iter == max_iters - 1) return SBR_NO_RUN_MAXITER;
        double xo = xnew;
        double ic = dmin(tin, xo), oc = dmin(tout, xo);
        double AW = INTERP(t, G, n, oc, &oob) - INTERP(t, G, n, ic, &oob);
        int64_t idx = ssl(t, n, xo);
        if (idx < 0 || idx + 1 >= n) return SBR_OOB;
        double eps = t[idx + 1] - t[idx];
        double AWe = INTERP(t, G, n, oc + eps, &oob) - INTERP(t, G, n, ic + eps, &oob);
        if (oob) return SBR_OOB;
        double err = AW - kappa;
        int inc = AWe >= AW;
        if (fabs(err) <= tolerance) {
            if (inc) { *xi_out = xo; *tol_out = fabs(err); return SBR_RUN; }
            return SBR_FALSE_EQ;
        } else if (err > 0) {
            xmax = xo;
            xnew = 0.5 * (xo + xmin);
        } else {
            xmin = xo;
            xnew = 0.5 * (xo + xmax);
        }
    }
    return SBR_NO_RUN_MAXITER;
}

/* ------------------------------------------------------------------------ */
/* get_AW on the HR grid + AW_max (solver.jl:495-532, 565)                  */
/* ------------------------------------------------------------------------ */
static double get_aw3(double xi, double tin, double tout, const double* tau, int64_t n_tau, const double* t,
                      const double* G, int64_t n, double* aw_path, double* aw_out_path, double* aw_in_path, int* oob)
{
    double ic = (tin >= xi) ? xi : tin;
    double oc = (tout > xi) ? xi : tout;
    double G0 = INTERP(t, G, n, 0.0, oob);
    double mx = -INFINITY;
    for (int64_t i = 0; i < n_tau; i++) {
        double a = (tau[i] - xi) + ic;
        double b = (tau[i] - xi) + oc;
        double gi = INTERP(t, G, n, a > 0 ? a : 0.0, oob);
        double go = INTERP(t, G, n, b > 0 ? b : 0.0, oob);
        double awin = a >= 0 ? gi : 0.0;
        double awout = b >= 0 ? go : 0.0;
        double v = (awout - awin) + G0;
        if (aw_path) aw_path[i] = v;
        if (aw_out_path) aw_out_path[i] = awout;
        if (aw_in_path) aw_in_path[i] = awin;
        if (mx == mx && (v != v || v > mx)) mx = v; /* NaN-propagating max (Julia maximum) */
    }
    return mx;
}

static double get_aw(double xi, double tin, double tout, const double* tau, int64_t n_tau, const double* t,
                     const double* G, int64_t n, double* aw_path, int* oob)
{
    return get_aw3(xi, tin, tout, tau, n_tau, t, G, n, aw_path, NULL, NULL, oob);
}

/* ------------------------------------------------------------------------ */
/* one (β, u) equilibrium given knots + hazard (solve_equilibrium_baseline)  */
/* ------------------------------------------------------------------------ */
typedef struct {
    double xi, tin, tout, aw_max, tol;
    uint32_t status;
    int32_t iters;
} point_t;

static void equilibrium_point3(const double* t, const double* G, int64_t n, const hazard_t* h, double t_end,
                               double u, double kappa, int32_t max_iters, point_t* r, double* aw_path,
                               double* aw_out_path, double* aw_in_path)
{
    memset(r, 0, sizeof(*r));
    r->xi = NAN;
    r->aw_max = NAN;
    r->tol = INFINITY;
    if (h->oob) { r->status = SBR_OOB; r->tin = r->tout = NAN; return; }
    optimal_buffer(u, h->tau, h->hr, h->n, t_end, &r->tin, &r->tout);
    if (r->tin == r->tout) {
        r->status = SBR_NO_RUN_HR_BELOW_U | SBR_CONVERGED;
        r->tol = 0.0;
        return;
    }
    double xi, tol;
    uint32_t s = compute_xi(r->tin, r->tout, t, G, n, kappa, max_iters, &xi, &tol, &r->iters);
    if (s != SBR_RUN) { r->status = s; return; }
    int oob = 0;
    double mx = get_aw3(xi, r->tin, r->tout, h->tau, h->n, t, G, n, aw_path, aw_out_path, aw_in_path, &oob);
    if (oob) { r->status = SBR_OOB; return; }
    r->xi = xi;
    r->tol = tol;
    r->aw_max = mx;
    r->status = SBR_RUN | SBR_CONVERGED;
}

static void equilibrium_point(const double* t, const double* G, int64_t n, const hazard_t* h, double t_end,
                              double u, double kappa, int32_t max_iters, point_t* r, double* aw_path)
{
    equilibrium_point3(t, G, n, h, t_end, u, kappa, max_iters, r, aw_path, NULL, NULL);
}

/* public single-point API on caller-provided knots (used by tests): solve_equilibrium_baseline on a
 * LearningResults' knots (solver.jl:413-462) + get_AW's three paths (solver.jl:495-532) */
/* the same on an explicit learning pdf's knot values g (hazard_rate(p, λ, pdf, η) for any pdf on
 * the knots, e.g. the social extension's (1 − G)·β·AW_{n−1}, social_learning_dynamics.jl:98-114) */
void sbro_equilibrium_paths_pdf(const double* t, const double* G, const double* g, int64_t n, double eta,
                                double t_end, double u, double p, double kappa, double lambda, int32_t max_iters,
                                double* res, uint32_t* status, int32_t* iters, double* hr_tau, double* hr_v,
                                double* aw, double* aw_out, double* aw_in, int64_t* n_hr)
{
    hazard_t h;
    hazard_rate(t, g, n, p, lambda, eta, 0, &h);
    point_t r;
    equilibrium_point3(t, G, n, &h, t_end, u, kappa, max_iters, &r, aw, aw_out, aw_in);
    res[0] = r.xi; res[1] = r.tin; res[2] = r.tout; res[3] = r.aw_max; res[4] = r.tol;
    *status = r.status;
    *iters = r.iters;
    if (n_hr) *n_hr = h.oob ? 0 : h.n;
    if (hr_tau && !h.oob) memcpy(hr_tau, h.tau, (size_t)h.n * sizeof(double));
    if (hr_v && !h.oob) memcpy(hr_v, h.hr, (size_t)h.n * sizeof(double));
    hazard_free(&h);
}

void sbro_equilibrium_paths(const double* t, const double* G, int64_t n, double beta, double eta, double t_end,
                            double u, double p, double kappa, double lambda, int32_t max_iters, double* res,
                            uint32_t* status, int32_t* iters, double* hr_tau, double* hr_v, double* aw,
                            double* aw_out, double* aw_in, int64_t* n_hr)
{
    double* g = (double*)malloc((size_t)n * sizeof(double));
    for (int64_t i = 0; i < n; i++) g[i] = (beta * G[i]) * (1.0 - G[i]);
    hazard_t h;
    hazard_rate(t, g, n, p, lambda, eta, 0, &h);
    point_t r;
    equilibrium_point3(t, G, n, &h, t_end, u, kappa, max_iters, &r, aw, aw_out, aw_in);
    res[0] = r.xi; res[1] = r.tin; res[2] = r.tout; res[3] = r.aw_max; res[4] = r.tol;
    *status = r.status;
    *iters = r.iters;
    if (n_hr) *n_hr = h.oob ? 0 : h.n;
    if (hr_tau && !h.oob) memcpy(hr_tau, h.tau, (size_t)h.n * sizeof(double));
    if (hr_v && !h.oob) memcpy(hr_v, h.hr, (size_t)h.n * sizeof(double));
    hazard_free(&h);
    free(g);
}

void sbro_equilibrium(const double* t, const double* G, int64_t n, double beta, double eta, double t_end,
                      double u, double p, double kappa, double lambda, int32_t max_iters, double* res,
                      uint32_t* status, int32_t* iters, double* hr_tau, double* hr_v, double* aw, int64_t* n_hr)
{
    double* g = (double*)malloc((size_t)n * sizeof(double));
    for (int64_t i = 0; i < n; i++) g[i] = (beta * G[i]) * (1.0 - G[i]);
    hazard_t h;
    hazard_rate(t, g, n, p, lambda, eta, 0, &h);
    point_t r;
    equilibrium_point(t, G, n, &h, t_end, u, kappa, max_iters, &r, aw);
    res[0] = r.xi; res[1] = r.tin; res[2] = r.tout; res[3] = r.aw_max; res[4] = r.tol;
    *status = r.status;
    *iters = r.iters;
    if (n_hr) *n_hr = h.n;
    if (hr_tau) memcpy(hr_tau, h.tau, (size_t)h.n * sizeof(double));
    if (hr_v) memcpy(hr_v, h.hr, (size_t)h.n * sizeof(double));
    hazard_free(&h);
    free(g);
}

/* ------------------------------------------------------------------------ */
/* Baseline β×u sweep (scripts/1_baseline.jl:224-267 without the early exit) */
/* learning + hazard once per β column (u-independent), then every u.       */
/* ------------------------------------------------------------------------ */
int sbro_sweep_baseline_opt(const double* beta, const double* eta, const double* t_end, double x0, const double* u,
                            int64_t n_beta, int64_t n_u, double p, double kappa, double lambda, int32_t max_iters,
                            int32_t nthreads, double* xi, double* tin, double* tout, double* aw_max, double* tol,
                            uint32_t* status, int32_t* iters, int64_t* nknots, double rtol, double atol,
                            int64_t ode_maxiters)
{
    int err = 0;
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(dynamic, 1) reduction(| : err)
#endif
    for (int64_t b = 0; b < n_beta; b++) {
        knots_t kn = {0};
        ode_stats_t st;
        ode_sys_t S;
        double x0v = x0;
        double bb = beta[b];
        if (ode_solve(sys_logistic(&bb, &S), 1, 0.0, t_end[b], &x0v, rtol, atol, ode_maxiters, &kn, &st)) {
            err |= 1;
            continue;
        }
        if (nknots) nknots[b] = kn.n;
        int64_t n = kn.n;
        double* g = (double*)malloc((size_t)n * sizeof(double));
        for (int64_t i = 0; i < n; i++) g[i] = (bb * kn.x[i]) * (1.0 - kn.x[i]);
        hazard_t h;
        hazard_rate(kn.t, g, n, p, lambda, eta[b], 0, &h);
        for (int64_t j = 0; j < n_u; j++) {
            point_t r;
            equilibrium_point(kn.t, kn.x, n, &h, t_end[b], u[j], kappa, max_iters, &r, NULL);
            int64_t o = b * n_u + j;
            xi[o] = r.xi; tin[o] = r.tin; tout[o] = r.tout; aw_max[o] = r.aw_max; tol[o] = r.tol;
            status[o] = r.status | (st.status & (SBR_ODE_MAXITERS | SBR_STIFF_SWITCH | SBR_ODE_FAILED));
            if (iters) iters[o] = r.iters;
        }
        hazard_free(&h);
        free(g);
        knots_free(&kn);
    }
    return err ? -1 : 0;
}

/* 5-consecutive-no-run early exit applied as a post-pass over u-fastest
 * columns (scripts/1_baseline.jl:236-244, :147-164).  Skipped points get
 * aw_max = xi = NaN, tol = Inf and SBR_SKIPPED_EARLY_EXIT. */
void sbro_apply_early_exit(int64_t n_beta, int64_t n_u, int32_t threshold, double* xi, double* aw_max, double* tol,
                           uint32_t* status)
{
    for (int64_t b = 0; b < n_beta; b++) {
        int32_t c = 0;
        for (int64_t j = 0; j < n_u; j++) {
            int64_t o = b * n_u + j;
            if (c >= threshold) {
                xi[o] = NAN; aw_max[o] = NAN; tol[o] = INFINITY;
                status[o] = SBR_SKIPPED_EARLY_EXIT;
                continue;
            }
            if (status[o] & SBR_RUN) c = 0;
            else c++;
        }
    }
}

/* FastPower.fastpower as the controller uses it (tests compare it against the device) */
void sbro_fastpow(const double* x, const double* y, int64_t n, double* out)
{
    for (int64_t i = 0; i < n; i++) out[i] = sbr_fastpow(x[i], y[i]);
}

/* detmath exports (tests compare them against numpy and against the device) */
void sbro_detmath(const double* x, const double* y, int64_t n, double* e, double* l, double* pw)
{
    for (int64_t i = 0; i < n; i++) {
        e[i] = sbr_exp(x[i]);
        l[i] = sbr_log(x[i]);
        pw[i] = sbr_pow_pos(x[i], y[i]);
    }
}

/* ======================================================================== */
/* Heterogeneity extension (K coupled groups)                               */
/* heterogeneity_learning.jl:49-134, heterogeneity_solver.jl:48-375         */
/* ======================================================================== */
typedef struct {
    int K;
    const double* betas;
    const double* dist;
} hetero_ctx;

/* ω = Σ_j dist_j I_j (generator sum: left fold from the first term);
 * du_k = (1 − I_k) β_k ω   (heterogeneity_learning.jl:57-67) */
static void rhs_hetero(void* ctx, double t, const double* I, double* du, int* oob)
{
    (void)t; (void)oob;
    const hetero_ctx* h = (const hetero_ctx*)ctx;
    double w = h->dist[0] * I[0];
    for (int j = 1; j < h->K; j++) w = w + h->dist[j] * I[j];
    for (int k = 0; k < h->K; k++) du[k] = ((1.0 - I[k]) * h->betas[k]) * w;
}

/* ForwardDiff jacobian of rhs_hetero: with b_k = (1 − I_k)·β_k (partials −β_k
 * in slot k) and ω (partials dist_j), the product rule gives
 * J_kj = dist_j·b_k (j ≠ k; the −0.0 partial adds nothing) and
 * J_kk = (−β_k)·ω + dist_k·b_k; autonomous: ∂f/∂t = 0 */
static void jac_hetero(void* ctx, double t, const double* I, double* J, double* dT, int* oob)
{
    (void)t; (void)oob;
    const hetero_ctx* h = (const hetero_ctx*)ctx;
    const int K = h->K;
    double w = h->dist[0] * I[0];
    for (int j = 1; j < K; j++) w = w + h->dist[j] * I[j];
    for (int k = 0; k < K; k++) {
        const double bk = (1.0 - I[k]) * h->betas[k];
        for (int j = 0; j < K; j++) J[k * K + j] = h->dist[j] * bk;
        J[k * K + k] = (-h->betas[k]) * w + h->dist[k] * bk;
        dT[k] = 0.0;
    }
}

int64_t sbro_learn_hetero_opt(const double* betas, const double* dist, int32_t K, double t1, double x0, double* t_out,
                              double* G_out, int64_t cap, int64_t* stats, double rtol, double atol,
                              int64_t ode_maxiters)
{
    knots_t kn = {0};
    ode_stats_t st;
    double x0v[MAXK];
    for (int k = 0; k < K; k++) x0v[k] = x0;
    hetero_ctx hc = {K, betas, dist};
    const ode_sys_t S = {rhs_hetero, K <= MAXJ ? jac_hetero : NULL, &hc};
    if (K < 1 || K > MAXK || ode_solve(&S, K, 0.0, t1, x0v, rtol, atol, ode_maxiters, &kn, &st)) {
        knots_free(&kn);
        return -1;
    }
    int64_t n = kn.n;
    if (stats) {
        stats[0] = st.naccept; stats[1] = st.nreject; stats[2] = st.status; stats[3] = n;
        memcpy(&stats[4], &st.t_switch, 8); stats[5] = st.nswitch; stats[6] = st.nstiff;
    }
    if (n > cap) n = -n;
    else {
        memcpy(t_out, kn.t, (size_t)kn.n * sizeof(double));
        memcpy(G_out, kn.x, (size_t)kn.n * K * sizeof(double));
    }
    knots_free(&kn);
    return n;
}

/* is_valid_equilibrium_hetero (heterogeneity_solver.jl:175-210) */
static int valid_hetero(double xs, const double* tin, const double* t, const double* G, int64_t n, int K,
                        double kappa, const double* dist, int* oob)
{
    int64_t m = 0;
    while (m < n && t[m] <= xs) m++;
    if (m == 0) return 1;
    int prev = 0;
    for (int64_t i = 0; i < m; i++) {
        double aw = 0.0;
        for (int k = 0; k < K; k++) {
            double tI = dmax(0.0, xs - tin[k]);
            double a = interp_s(t, G + k, K, n, t[i], oob);
            double b = interp_s(t, G + k, K, n, dmax(0.0, t[i] - tI), oob);
            aw = aw + dist[k] * (a - b);
        }
        int above = aw > kappa;
        /* any i with above[i] && !above[i+1] (the reference scans backwards; same set) */
        if (i > 0 && prev && !above) return 0;
        prev = above;
    }
    return 1;
}

/* compute_ξ_hetero (heterogeneity_solver.jl:48-144) */
static uint32_t compute_xi_hetero(const double* tin, const double* tout, const double* dist, int K, const double* t,
                                  const double* G, int64_t n, double kappa, int32_t max_iters, double tolerance,
                                  double* xi_out, double* tol_out, int32_t* iters)
{
    int oob = 0;
    double guess = (dist[0] * (tin[0] + tout[0])) / 2.0;
    for (int k = 1; k < K; k++) guess = guess + (dist[k] * (tin[k] + tout[k])) / 2.0;
    double mo = tout[0];
    for (int k = 1; k < K; k++) mo = dmax(mo, tout[k]);
    double xmin = 0.0, xmax = mo * 2.0, xnew = guess;
    *xi_out = NAN;
    *tol_out = INFINITY;
    for (int32_t iter = 1; iter <= max_iters; iter++) {
        *iters = iter;
        double d = xmin - xmax;
        if (fabs(d) < 2.0 * sbr_jl_eps(d)) return SBR_NO_RUN_COLLAPSE;
        if (iter == max_iters - 1) return SBR_NO_RUN_MAXITER;
        double xo = xnew;
        int64_t idx = ssl(t, n, xo);
        if (idx < 0) return SBR_OOB;
        int64_t i2 = idx + 1 < n - 1 ? idx + 1 : n - 1; /* min(current_idx + 1, length) */
        double eps = t[i2] - t[idx];
        double AW = 0.0, AWe = 0.0;
        for (int k = 0; k < K; k++) {
            double ic = dmin(tin[k], xo), oc = dmin(tout[k], xo);
            AW = AW + dist[k] * (interp_s(t, G + k, K, n, oc, &oob) - interp_s(t, G + k, K, n, ic, &oob));
            AWe = AWe + dist[k] * (interp_s(t, G + k, K, n, oc + eps, &oob) -
                                   interp_s(t, G + k, K, n, ic + eps, &oob));
        }
        if (oob) return SBR_OOB;
        double err = AW - kappa;
        int inc = AWe >= AW;
        if (fabs(err) <= tolerance) {
            if (inc) {
                int v = valid_hetero(xo, tin, t, G, n, K, kappa, dist, &oob);
                if (oob) return SBR_OOB;
                if (!v) return SBR_HETERO_INVALID;
                *xi_out = xo;
                *tol_out = fabs(err);
                return SBR_RUN;
            }
            return SBR_FALSE_EQ;
        } else if (err > 0) {
            xmax = xo;
            xnew = 0.5 * (xo + xmin);
        } else {
            xmin = xo;
            xnew = 0.5 * (xo + xmax);
        }
    }
    return SBR_NO_RUN_MAXITER;
}

/* get_AW_hetero's AW_max over the whole learning grid (heterogeneity_solver.jl:316-375) */
/* get_AW_hetero (heterogeneity_solver.jl:316-375) on the knots: AW_cum into cum[n], returns its
 * maximum; grp (may be NULL): the per-group AW_OUT_k at grp + k·ld, AW_IN_k at grp + (K + k)·ld */
static double aw_max_hetero_groups(double xi, const double* tin, const double* tout, const double* dist, int K,
                                   const double* t, const double* G, int64_t n, double* cum, int* oob, double* grp,
                                   int64_t ld)
{
    for (int64_t i = 0; i < n; i++) cum[i] = 0.0;
    for (int k = 0; k < K; k++) {
        double ic = dmin(tin[k], xi), oc = dmin(tout[k], xi);
        for (int64_t i = 0; i < n; i++) {
            double a = (t[i] - xi) + ic;
            double b = (t[i] - xi) + oc;
            double gi = interp_s(t, G + k, K, n, a > 0 ? a : 0.0, oob);
            double go = interp_s(t, G + k, K, n, b > 0 ? b : 0.0, oob);
            double awin = a >= 0 ? gi : 0.0;
            double awout = b >= 0 ? go : 0.0;
            cum[i] = cum[i] + dist[k] * (awout - awin);
            if (grp) {
                grp[(int64_t)k * ld + i] = awout;
                grp[(int64_t)(K + k) * ld + i] = awin;
            }
        }
    }
    double mx = -INFINITY;
    for (int64_t i = 0; i < n; i++)
        if (mx == mx && (cum[i] != cum[i] || cum[i] > mx)) mx = cum[i];
    return mx;
}

static double aw_max_hetero(double xi, const double* tin, const double* tout, const double* dist, int K,
                            const double* t, const double* G, int64_t n, double* cum, int* oob)
{
    return aw_max_hetero_groups(xi, tin, tout, dist, K, t, G, n, cum, oob, NULL, 0);
}

/* Hetero sweep: column c has group rates betas[c*K .. c*K+K), η = eta[c],
 * tspan = (0, t_end[c]); every u.  Outputs u-fastest; tin/tout are [pt][K]. */
/* heterogeneity_solver.jl:241-293 + get_AW_hetero on one column's knots (t[n], I[n][K]):
 * compute_pdf_hetero, the K hazards on the explicit grid, then per u the buffers, compute_ξ_hetero
 * and AW_max.  hr_out (may be NULL): HR_k on the τ̄ grid at hr_out + k·(n+1) (*n_hr entries, 0
 * after a BoundsError); aw_path (may be NULL, n_u = 1): AW_total on the knots. */
static void hetero_column(int32_t K, const double* bk, const double* dist, const double* t, const double* I,
                          int64_t n, double eta, double t_end, const double* u, int64_t n_u, double p, double kappa,
                          double lambda, int32_t max_iters, double tolerance, uint32_t lbits, double* xi,
                          double* aw_max, double* tol, uint32_t* status, int32_t* iters, double* tin_out,
                          double* tout_out, double* hr_out, int64_t* n_hr, double* aw_path)
{
    /* compute_pdf_hetero: pdf_k = (1 − I_k) β_k ω at the knots */
    double* g = (double*)malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
    double* cum = (double*)malloc((size_t)(n > 0 ? n : 1) * sizeof(double));
    hazard_t hz[MAXK];
    int hz_oob = 0;
    for (int k = 0; k < K; k++) {
        for (int64_t i = 0; i < n; i++) {
            const double* Ii = I + i * K;
            double w = dist[0] * Ii[0];
            for (int j = 1; j < K; j++) w = w + dist[j] * Ii[j];
            g[i] = ((1.0 - Ii[k]) * bk[k]) * w;
        }
        hazard_rate(t, g, n, p, lambda, eta, 1, &hz[k]);
        hz_oob |= hz[k].oob;
    }
    if (n_hr) *n_hr = hz_oob ? 0 : hz[0].n;
    if (hr_out && !hz_oob)
        for (int k = 0; k < K; k++) memcpy(hr_out + (size_t)k * (n + 1), hz[k].hr, (size_t)hz[k].n * sizeof(double));
    for (int64_t j = 0; j < n_u; j++) {
        double tin[MAXK], tout[MAXK];
        uint32_t s = 0;
        double x = NAN, tl = INFINITY, am = NAN;
        int32_t it = 0;
        if (hz_oob) {
            s = SBR_OOB;
            for (int k = 0; k < K; k++) tin[k] = tout[k] = NAN;
        } else {
            int all_eq = 1;
            for (int k = 0; k < K; k++) {
                optimal_buffer(u[j], hz[k].tau, hz[k].hr, hz[k].n, t_end, &tin[k], &tout[k]);
                all_eq &= (tin[k] == tout[k]);
            }
            if (all_eq) {
                s = SBR_NO_RUN_HR_BELOW_U | SBR_CONVERGED;
                tl = 0.0;
            } else {
                s = compute_xi_hetero(tin, tout, dist, K, t, I, n, kappa, max_iters, tolerance, &x, &tl, &it);
                if (s == SBR_RUN) {
                    int oob = 0;
                    am = aw_max_hetero(x, tin, tout, dist, K, t, I, n, aw_path ? aw_path : cum, &oob);
                    if (oob) { s = SBR_OOB; x = NAN; tl = INFINITY; am = NAN; }
                    else s = SBR_RUN | SBR_CONVERGED;
                }
            }
        }
        xi[j] = x; tol[j] = tl; aw_max[j] = am;
        status[j] = s | lbits;
        if (iters) iters[j] = it;
        for (int k = 0; k < K; k++) {
            if (tin_out) tin_out[j * K + k] = tin[k];
            if (tout_out) tout_out[j * K + k] = tout[k];
        }
    }
    for (int k = 0; k < K; k++) hazard_free(&hz[k]);
    free(g);
    free(cum);
}

int sbro_sweep_hetero_opt(int32_t K, const double* betas, const double* dist, const double* eta, const double* t_end,
                          double x0, const double* u, int64_t n_col, int64_t n_u, double p, double kappa, double lambda,
                          int32_t max_iters, double tolerance, int32_t nthreads, double* xi, double* aw_max,
                          double* tol, uint32_t* status, int32_t* iters, double* tin_out, double* tout_out,
                          int64_t* nknots, double rtol, double atol, int64_t ode_maxiters)
{
    int err = 0;
    if (K < 1 || K > MAXK) return -1;
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(dynamic, 1) reduction(| : err)
#endif
    for (int64_t c = 0; c < n_col; c++) {
        const double* bk = betas + c * K;
        knots_t kn = {0};
        ode_stats_t st;
        double x0v[MAXK];
        for (int k = 0; k < K; k++) x0v[k] = x0;
        hetero_ctx hc = {K, bk, dist};
        const ode_sys_t S = {rhs_hetero, K <= MAXJ ? jac_hetero : NULL, &hc};
        if (ode_solve(&S, K, 0.0, t_end[c], x0v, rtol, atol, ode_maxiters, &kn, &st)) { err |= 1; continue; }
        if (nknots) nknots[c] = kn.n;
        const int64_t o = c * n_u;
        hetero_column(K, bk, dist, kn.t, kn.x, kn.n, eta[c], t_end[c], u, n_u, p, kappa, lambda, max_iters, tolerance,
                      st.status & (SBR_ODE_MAXITERS | SBR_STIFF_SWITCH | SBR_ODE_FAILED), xi + o, aw_max + o, tol + o,
                      status + o, iters ? iters + o : NULL, tin_out ? tin_out + o * K : NULL,
                      tout_out ? tout_out + o * K : NULL, NULL, NULL, NULL);
        knots_free(&kn);
    }
    return err ? -1 : 0;
}

/* solve_equilibrium_hetero(lr_hetero, econ) on caller knots (a LearningResultsHetero's grid and
 * group CDFs, I[n][K]) for n_u values of u; hr_out [K][n+1], aw_path [n] (n_u = 1) may be NULL */
void sbro_hetero_equilibrium_knots(int32_t K, const double* t, const double* I, int64_t n, const double* betas,
                                   const double* dist, double eta, double t_end, const double* u, int64_t n_u,
                                   double p, double kappa, double lambda, double* xi, double* aw_max, double* tol,
                                   uint32_t* status, int32_t* iters, double* tin, double* tout, double* hr_out,
                                   int64_t* n_hr, double* aw_path)
{
    hetero_column(K, betas, dist, t, I, n, eta, t_end, u, n_u, p, kappa, lambda, 500, 1e-12, 0, xi, aw_max, tol,
                  status, iters, tin, tout, hr_out, n_hr, aw_path);
}

/* ======================================================================== */
/* Social-learning extension: endogenous learning fixed point               */
/* social_learning_dynamics.jl:58-114, social_learning_solver.jl:63-263     */
/* ======================================================================== */
typedef struct {
    double beta;
    const double* t; /* AW_old knots */
    const double* v; /* AW_old values */
    int64_t n;
} social_ctx;

/* ODE_social_learning!: du = (1 − I) β AW_old(t)  (social_learning_dynamics.jl:61-67);
 * AW_old(t) is a Throw()-extrapolating LinearInterpolation (BoundsError -> oob) */
static void rhs_social(void* ctx, double t, const double* x, double* dx, int* oob)
{
    const social_ctx* s = (const social_ctx*)ctx;
    double aw = interp_s(s->t, s->v, 1, s->n, t, oob);
    dx[0] = ((1.0 - x[0]) * s->beta) * aw;
}

/* ForwardDiff: J = ((−1)·β)·AW_old(t); ∂f/∂t = ((1 − I)·β)·AW_old'(t) with the
 * interpolant's dual-number slope (interp_dx) */
static void jac_social(void* ctx, double t, const double* x, double* J, double* dT, int* oob)
{
    const social_ctx* s = (const social_ctx*)ctx;
    const double aw = interp_s(s->t, s->v, 1, s->n, t, oob);
    const double awp = interp_dx(s->t, s->v, 1, s->n, t, oob);
    J[0] = ((-1.0) * s->beta) * aw;
    dT[0] = ((1.0 - x[0]) * s->beta) * awp;
}

/* One (β, u) point of solve_equilibrium_social_learning (social_learning_solver.jl:63-263).
 * tspan = (0, η) (:79); cmp = range(0, η, length=n_cmp) supplied by the caller
 * (:103).  Returns the last inner SolvedModel's fields (:262) like the
 * reference; the fixed-point outcome goes to SBR_SOCIAL_NOT_CONVERGED and
 * *fp_iters.  stats (may be NULL) = {ODE knots of the last iterate, Σ accepted
 * steps, Σ rejected steps, max knots over iterates}. */
typedef struct {
    double *t, *G, *tau; /* last iterate's learning knots and HR grid (caller-allocated, cap each) */
    double* awo;         /* AW_{n-1} at those knots: the forcing of learning_pdf (may be NULL) */
    int64_t cap, n, n_tau;
} social_paths_t;

static void social_point(double beta, double eta, double x0, double u, double p, double kappa, double lambda,
                         const double* cmp, int32_t n_cmp, double tol, int32_t max_iter, int32_t bisect_max_iters,
                         double rtol, double atol, int64_t ode_maxiters, point_t* out, int32_t* fp_iters,
                         int64_t* stats, social_paths_t* paths)
{
    memset(out, 0, sizeof(*out));
    out->xi = NAN; out->aw_max = NAN; out->tol = INFINITY; out->tin = out->tout = NAN;
    *fp_iters = 0;
    int64_t s_acc = 0, s_rej = 0, s_max = 0;
    uint32_t ode_bits = 0;
    /* initial guess: baseline SI learning on (0, η); AW_old = G on its knots (:89-94) */
    knots_t old = {0};
    ode_stats_t st;
    ode_sys_t S0;
    double x0v = x0, bb = beta;
    if (ode_solve(sys_logistic(&bb, &S0), 1, 0.0, eta, &x0v, rtol, atol, ode_maxiters, &old, &st)) {
        out->status = SBR_ODE_FAILED; knots_free(&old); return;
    }
    ode_bits |= st.status & (SBR_ODE_MAXITERS | SBR_STIFF_SWITCH | SBR_ODE_FAILED | SBR_OOB);
    double xi_new = 0.0;
    int converged = 0, have_result = 0, stop_oob = 0;
    int32_t iter;
    for (iter = 1; iter <= max_iter; iter++) {
        double xi_old = xi_new;
        /* (a) learning from withdrawals: tspan (0, η), eps tolerances (:128-130) */
        knots_t kn = {0};
        social_ctx sc = {beta, old.t, old.x, old.n};
        const ode_sys_t S = {rhs_social, jac_social, &sc};
        x0v = x0;
        if (ode_solve(&S, 1, 0.0, eta, &x0v, rtol, atol, ode_maxiters, &kn, &st)) {
            out->status = SBR_ODE_FAILED; knots_free(&kn); break;
        }
        s_acc += st.naccept; s_rej += st.nreject;
        if (kn.n > s_max) s_max = kn.n;
        if (getenv("SBRO_DEBUG"))
            fprintf(stderr, "social it %d: knots %ld acc %ld rej %ld status %x\n", iter, (long)kn.n, (long)st.naccept,
                    (long)st.nreject, st.status);
        ode_bits |= st.status & (SBR_ODE_MAXITERS | SBR_STIFF_SWITCH | SBR_ODE_FAILED);
        if (st.status & SBR_OOB) { stop_oob = 1; knots_free(&kn); break; }
        int64_t n = kn.n;
        /* compute_pdf_social_learning (:98-114): g = (1 − G) β AW_old(t) at the knots */
        double* awo = (double*)malloc((size_t)n * sizeof(double));
        double* g = (double*)malloc((size_t)n * sizeof(double));
        int oob = 0;
        for (int64_t i = 0; i < n; i++) {
            awo[i] = interp_s(old.t, old.x, 1, old.n, kn.t[i], &oob);
            g[i] = ((1.0 - kn.x[i]) * beta) * awo[i];
        }
        /* (b) baseline equilibrium on the new learning; t_end = tspan[2] = η (:139-143) */
        hazard_t h;
        hazard_rate(kn.t, g, n, p, lambda, eta, 0, &h);
        h.oob |= oob;
        point_t r;
        double* aw = (double*)malloc((size_t)h.n * sizeof(double));
        equilibrium_point(kn.t, kn.x, n, &h, eta, u, kappa, bisect_max_iters, &r, aw);
        *out = r;
        have_result = 1;
        if (paths) {
            paths->n = n; paths->n_tau = h.n;
            if (n <= paths->cap && h.n <= paths->cap) {
                memcpy(paths->t, kn.t, (size_t)n * sizeof(double));
                memcpy(paths->G, kn.x, (size_t)n * sizeof(double));
                memcpy(paths->tau, h.tau, (size_t)h.n * sizeof(double));
                if (paths->awo) memcpy(paths->awo, awo, (size_t)n * sizeof(double));
            }
        }
        if (r.status & SBR_OOB) { stop_oob = 1; }
        else {
            int stop = 0;
            if (!(r.status & SBR_RUN)) {
                /* no equilibrium with this learning: ξ += η/500 (:150-156) */
                xi_new = xi_old + eta / 500.0;
                if (xi_new > eta) stop = 1;
                else get_aw(xi_new, r.tin, r.tout, h.tau, h.n, kn.t, kn.x, n, aw, &oob);
            } else {
                xi_new = r.xi; /* aw already holds get_AW(ξ, …) on the HR grid */
            }
            if (oob) stop_oob = 1;
            if (!stop && !stop_oob) {
                /* ∞-norm on the comparison grid, before damping (:162-163, :195-196) */
                double err = 0.0;
                for (int32_t k = 0; k < n_cmp; k++) {
                    double d = fabs(interp_s(h.tau, aw, 1, h.n, cmp[k], &oob) -
                                    interp_s(old.t, old.x, 1, old.n, cmp[k], &oob));
                    if (k == 0) err = d;
                    else if (!(err != err || err > d)) err = d; /* generic_normInf: NaN sticks */
                }
                if (getenv("SBRO_DEBUG")) fprintf(stderr, "social it %d: err %.6e xi %.6f\n", iter, err, xi_new);
                if (oob) stop_oob = 1;
                else if (err < tol) {
                    converged = 1;
                } else {
                    /* damping α = 1/2 on the new knots (:174-178, :218-222) */
                    for (int64_t i = 0; i < n; i++) {
                        double vn = interp_s(h.tau, aw, 1, h.n, kn.t[i], &oob);
                        awo[i] = 0.5 * awo[i] + 0.5 * vn;
                    }
                    if (oob) stop_oob = 1;
                    knots_free(&old);
                    old.t = kn.t; old.x = awo; old.n = n; old.cap = kn.cap; old.K = 1;
                    kn.t = NULL; awo = NULL;
                }
            }
            if (stop) { free(aw); free(g); free(awo); hazard_free(&h); knots_free(&kn); break; }
        }
        free(aw); free(g); free(awo);
        hazard_free(&h);
        knots_free(&kn);
        if (converged || stop_oob) break;
    }
    if (iter > max_iter) iter = max_iter;
    *fp_iters = iter;
    knots_free(&old);
    if (stop_oob || !have_result) {
        out->xi = NAN; out->aw_max = NAN; out->tol = INFINITY;
        out->status = (out->status & ~(SBR_RUN | SBR_CONVERGED)) | SBR_OOB;
    }
    out->status |= ode_bits;
    if (!converged) out->status |= SBR_SOCIAL_NOT_CONVERGED;
    if (stats) { stats[0] = s_max; stats[1] = s_acc; stats[2] = s_rej; stats[3] = s_max; }
}

/* Social sweep over β columns × u; column b has η = eta[b]; cmp is
 * [n_beta][n_cmp] (the caller's range(0, η_b, length = n_cmp)). */
int sbro_sweep_social_opt(const double* beta, const double* eta, double x0, const double* u, int64_t n_beta,
                          int64_t n_u, double p, double kappa, double lambda, const double* cmp, int32_t n_cmp,
                          double tol, int32_t max_iter, int32_t bisect_max_iters, int32_t nthreads, double* xi,
                          double* tin, double* tout, double* aw_max, double* tl, uint32_t* status, int32_t* iters,
                          int32_t* fp_iters, int64_t* stats, double rtol, double atol, int64_t ode_maxiters)
{
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(dynamic, 1)
#endif
    for (int64_t o = 0; o < n_beta * n_u; o++) {
        int64_t b = o / n_u, j = o % n_u;
        point_t r;
        int32_t fi;
        social_point(beta[b], eta[b], x0, u[j], p, kappa, lambda, cmp + b * n_cmp, n_cmp, tol, max_iter,
                     bisect_max_iters, rtol, atol, ode_maxiters, &r, &fi, stats ? stats + 4 * o : NULL, NULL);
        xi[o] = r.xi; tin[o] = r.tin; tout[o] = r.tout; aw_max[o] = r.aw_max; tl[o] = r.tol;
        status[o] = r.status;
        if (iters) iters[o] = r.iters;
        if (fp_iters) fp_iters[o] = fi;
    }
    return 0;
}

/* single social point with the last iterate's paths (learning knots t/G and the
 * HR grid τ̄) for the figure checks; res = {ξ, τ̄_IN, τ̄_OUT, AW_max, tol}.
 * Returns the knot count (negative -needed if cap is too small). */
int64_t sbro_social_point_opt(double beta, double eta, double x0, double u, double p, double kappa, double lambda,
                              const double* cmp, int32_t n_cmp, double tol, int32_t max_iter, double* res,
                              uint32_t* status, int32_t* fp_iters, double* t_out, double* G_out, double* tau_out,
                              double* awo_out, int64_t cap, int64_t* n_tau, double rtol, double atol,
                              int64_t ode_maxiters)
{
    social_paths_t sp = {t_out, G_out, tau_out, awo_out, cap, 0, 0};
    point_t r;
    social_point(beta, eta, x0, u, p, kappa, lambda, cmp, n_cmp, tol, max_iter, 100, rtol, atol, ode_maxiters, &r,
                 fp_iters, NULL, &sp);
    res[0] = r.xi; res[1] = r.tin; res[2] = r.tout; res[3] = r.aw_max; res[4] = r.tol;
    *status = r.status;
    *n_tau = sp.n_tau;
    return (sp.n > cap || sp.n_tau > cap) ? -(sp.n > sp.n_tau ? sp.n : sp.n_tau) : sp.n;
}

/* one hetero point with its paths (aggregate_withdrawals_hetero.pdf): res = {ξ, AW_max, tol};
 * learning knots t[n], G[n][K], per-group buffers, AW_total on the knots and (aw_groups, may be
 * NULL) AW_OUT_k / AW_IN_k at rows k / K + k of stride cap — NaN without a run */
int64_t sbro_hetero_point_paths_opt(int32_t K, const double* betas, const double* dist, double eta, double t_end,
                                    double x0, double u, double p, double kappa, double lambda, double* res,
                                    uint32_t* status, double* tin, double* tout, double* t_out, double* G_out,
                                    double* aw_out, double* aw_groups, int64_t cap, double rtol, double atol,
                                    int64_t ode_maxiters)
{
    int32_t it = 0;
    int64_t nk = 0;
    if (sbro_sweep_hetero_opt(K, betas, dist, &eta, &t_end, x0, &u, 1, 1, p, kappa, lambda, 500, 1e-12, 1, &res[0],
                          &res[1], &res[2], status, &it, tin, tout, &nk, rtol, atol, ode_maxiters))
        return -1;
    const int64_t n =
        sbro_learn_hetero_opt(betas, dist, K, t_end, x0, t_out, G_out, cap, NULL, rtol, atol, ode_maxiters);
    if (n < 0) return n;
    if (*status & SBR_RUN) {
        int oob = 0;
        (void)aw_max_hetero_groups(res[0], tin, tout, dist, K, t_out, G_out, n, aw_out, &oob, aw_groups, cap);
    } else {
        for (int64_t i = 0; i < n; i++) aw_out[i] = NAN;
        for (int64_t r = 0; aw_groups && r < 2 * K; r++)
            for (int64_t i = 0; i < n; i++) aw_groups[r * cap + i] = NAN;
    }
    return n;
}

/* ------------------------------------------------------------------------ */
/* Interest-rate extension (src/extensions/interest_rates/)                  */
/* ------------------------------------------------------------------------ */
/* Tsit5 dense-output coefficients (OrdinaryDiffEqTsit5 Tsit5Interp; not
 * vendored).  Check: b_i(Θ=1) sums to the tableau's last row A7i (b7(1) = 0). */
static const double R11 = 1.0, R12 = -2.763706197274826, R13 = 2.9132554618219126, R14 = -1.0530884977290216;
static const double R22 = 0.13169999999999998, R23 = -0.2234, R24 = 0.1017;
static const double R32 = 3.9302962368947516, R33 = -5.941033872131505, R34 = 2.490627285651253;
static const double R42 = -12.411077166933676, R43 = 30.33818863028232, R44 = -16.548102889244902;
static const double R52 = 37.50931341651104, R53 = -88.1789048947664, R54 = 47.37952196281928;
static const double R62 = -27.896526289197286, R63 = 65.09189467479366, R64 = -34.87065786149660;
static const double R72 = 1.5, R73 = -4.0, R74 = 2.5;

/* _ode_interpolant(Θ, dt, y0, y1, k, ::Tsit5Cache, nothing, Val{0}) under
 * @muladd: Horner polynomials (evalpoly → muladd) and the 7-term sum nested
 * as muladd(k1, b1Θ, muladd(k2, b2Θ, … muladd(k6, b6Θ, k7·b7Θ))). */
static double tsit5_dense(double th, double dt, double y0, const double* const* k)
{
    const double th2 = th * th;
    const double b1 = th * fma(th, fma(th, fma(th, R14, R13), R12), R11);
    const double b2 = th2 * fma(th, fma(th, R24, R23), R22);
    const double b3 = th2 * fma(th, fma(th, R34, R33), R32);
    const double b4 = th2 * fma(th, fma(th, R44, R43), R42);
    const double b5 = th2 * fma(th, fma(th, R54, R53), R52);
    const double b6 = th2 * fma(th, fma(th, R64, R63), R62);
    const double b7 = th2 * fma(th, fma(th, R74, R73), R72);
    const double sum = fma(k[0][0], b1, fma(k[1][0], b2, fma(k[2][0], b3, fma(k[3][0], b4,
                           fma(k[4][0], b5, fma(k[5][0], b6, k[6][0] * b7))))));
    return fma(dt, sum, y0);
}

typedef struct {
    const double* tau; /* HR grid τ̄ */
    const double* hr;
    int64_t n;
    double delta, r, u;
} vf_ctx;

/* hjb_equation! (value_function_solver.jl:86-95):
 * dV = (h + δ)(1 − V) + max(u + rV − h, 0), h = HR(τ̄) (Throw() outside the grid) */
static void rhs_value(void* ctx, double t, const double* V, double* dV, int* oob)
{
    const vf_ctx* c = (const vf_ctx*)ctx;
    const double h = INTERP(c->tau, c->hr, c->n, t, oob);
    const double x = (c->u + c->r * V[0]) - h;
    const double re = (x != x) ? x : (x > 0.0 ? x : 0.0); /* Julia max(x, 0.0): NaN wins, max(-0.0, 0.0) = 0.0 */
    dV[0] = (h + c->delta) * (1.0 - V[0]) + re;
}

/* ForwardDiff: max(x, 0.0) on a Dual keeps x (and its partials) iff 0 < x
 * (isless), else the constant 0.0; J = −(h + δ) + (r | 0),
 * ∂f/∂τ̄ = h'·(1 − V) + (−h' | 0) with h' the HR interpolant's slope */
static void jac_value(void* ctx, double t, const double* V, double* J, double* dT, int* oob)
{
    const vf_ctx* c = (const vf_ctx*)ctx;
    const double h = INTERP(c->tau, c->hr, c->n, t, oob);
    const double hp = interp_dx(c->tau, c->hr, 1, c->n, t, oob);
    const double x = (c->u + c->r * V[0]) - h;
    const int keep = (x != x) || (x > 0.0);
    J[0] = (h + c->delta) * (-1.0) + (keep ? c->r : 0.0);
    dT[0] = hp * (1.0 - V[0]) + (keep ? -hp : 0.0);
}

typedef struct {
    const double* grid; /* saveat = the HR grid */
    int64_t n, next;
    double* V;
} saveat_t;

/* savevalues! with saveat: every pending point ≤ t, interpolated at
 * Θ = (s − tprev)/dt unless it is t itself (then the step's u) */
/* Rosenbrock23's dense output (_ode_interpolant, @muladd):
 * y0 + dt·(c1·k1 + c2·k2), c1 = Θ(1 − Θ)/(1 − 2d), c2 = Θ(Θ − 2d)/(1 − 2d) */
static double ros23_dense(double th, double dt, double y0, const double* const* k)
{
    const double omd = 1.0 - 2.0 * ROS23_D;
    const double c1 = (th * (1.0 - th)) / omd;
    const double c2 = (th * fma(-2.0, ROS23_D, th)) / omd;
    return fma(dt, fma(c1, k[0][0], c2 * k[1][0]), y0);
}

static void saveat_step(void* ctx, double tprev, double t, double dt, const double* y0, const double* y1,
                        const double* const* k, int stiff)
{
    saveat_t* s = (saveat_t*)ctx;
    while (s->next < s->n && s->grid[s->next] <= t) {
        const double ts = s->grid[s->next];
        const double th = (ts - tprev) / dt;
        s->V[s->next++] = (ts != t) ? (stiff ? ros23_dense(th, dt, y0[0], k) : tsit5_dense(th, dt, y0[0], k)) : y1[0];
    }
}

/* solve_value_function(hr, δ, r, u; tol) on the HR grid (the reference's tol = eps()); returns the
 * saved prefix length (== n unless the solve stopped early), V[0..) values */
static int64_t value_function(const hazard_t* h, double delta, double r, double u, double rtol, double atol,
                              int64_t maxiters, double* V, ode_stats_t* st)
{
    vf_ctx c = {h->tau, h->hr, h->n, delta, r, u};
    const double V0 = (u + delta) / (r + delta);
    saveat_t sv = {h->tau, h->n, 1, V};
    V[0] = V0; /* save_start: τ̄_1 = 0 = tspan[1] */
    const ode_sys_t S = {rhs_value, jac_value, &c};
    ode_solve_cb(&S, 1, 0.0, h->tau[h->n - 1], &V0, rtol, atol, maxiters, NULL, st, saveat_step, &sv);
    return sv.next;
}

/* solve_equilibrium_interest (interest_rate_solver.jl:51-150) for one u given
 * the learning knots and the hazard; V_out (may be NULL) receives V on the grid */
static void interest_point(const double* t, const double* G, int64_t n, const hazard_t* h, double t_end, double u,
                           double kappa, double r, double delta, int32_t max_iters, double rtol, double atol,
                           int64_t ode_maxiters, point_t* res, double* V_out, int64_t* n_v, int64_t* steps,
                           double* aw_path)
{
    memset(res, 0, sizeof(*res));
    res->xi = NAN;
    res->aw_max = NAN;
    res->tol = INFINITY;
    if (n_v) *n_v = 0;
    if (steps) *steps = 0;
    if (h->oob) { res->status = SBR_OOB; res->tin = res->tout = NAN; return; }
    uint32_t bits = 0;
    if (r > 0.0) {
        double* V = (double*)malloc((size_t)h->n * sizeof(double));
        double* hv = (double*)malloc((size_t)h->n * sizeof(double));
        ode_stats_t st;
        const int64_t ns = value_function(h, delta, r, u, rtol, atol, ode_maxiters, V, &st);
        bits = st.status & (SBR_ODE_MAXITERS | SBR_STIFF_SWITCH | SBR_ODE_FAILED | SBR_OOB);
        if (steps) *steps = st.naccept + st.nreject;
        if (n_v) *n_v = ns;
        if (V_out) memcpy(V_out, V, (size_t)ns * sizeof(double));
        /* h_rV on V's knots (= the saved grid): HR(t) − r·V(t), both interpolants
         * evaluated at their own knots (interest_rate_solver.jl:88-90) */
        int oob = 0;
        for (int64_t i = 0; i < ns; i++)
            hv[i] = INTERP(h->tau, h->hr, h->n, h->tau[i], &oob) - r * INTERP(h->tau, V, ns, h->tau[i], &oob);
        if (oob || (bits & SBR_OOB)) {
            res->status = SBR_OOB | bits;
            res->tin = res->tout = NAN;
            free(V); free(hv);
            return;
        }
        optimal_buffer(u, h->tau, hv, ns, t_end, &res->tin, &res->tout);
        free(V);
        free(hv);
    } else {
        optimal_buffer(u, h->tau, h->hr, h->n, t_end, &res->tin, &res->tout);
    }
    if (res->tin == res->tout) {
        res->status = SBR_NO_RUN_HR_BELOW_U | SBR_CONVERGED | bits;
        res->tol = 0.0;
        return;
    }
    double xi, tol;
    uint32_t s = compute_xi(res->tin, res->tout, t, G, n, kappa, max_iters, &xi, &tol, &res->iters);
    if (s != SBR_RUN) { res->status = s | bits; return; }
    int oob = 0;
    double mx = get_aw(xi, res->tin, res->tout, h->tau, h->n, t, G, n, aw_path, &oob);
    if (oob) { res->status = SBR_OOB | bits; return; }
    res->xi = xi;
    res->tol = tol;
    res->aw_max = mx;
    res->status = SBR_RUN | SBR_CONVERGED | bits;
}

/* β × u sweep of the interest-rate equilibrium: learning + hazard per β
 * column (as the baseline), then the value function and equilibrium per u. */
int sbro_sweep_interest_opt(const double* beta, const double* eta, const double* t_end, double x0, const double* u,
                            int64_t n_beta, int64_t n_u, double p, double kappa, double lambda, double r, double delta,
                            int32_t max_iters, int32_t nthreads, double* xi, double* tin, double* tout, double* aw_max,
                            double* tol, uint32_t* status, int32_t* iters, int64_t* steps, double rtol, double atol,
                            int64_t ode_maxiters)
{
    int rc = 0;
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(dynamic, 1) reduction(| : rc)
#endif
    for (int64_t b = 0; b < n_beta; b++) {
        knots_t kn = {0};
        ode_stats_t st;
        ode_sys_t S;
        double bt = beta[b];
        if (ode_solve(sys_logistic(&bt, &S), 1, 0.0, t_end[b], &x0, rtol, atol, ode_maxiters, &kn, &st)) {
            rc |= 1;
            continue;
        }
        double* g = (double*)malloc((size_t)kn.n * sizeof(double));
        for (int64_t i = 0; i < kn.n; i++) g[i] = (bt * kn.x[i]) * (1.0 - kn.x[i]);
        hazard_t h;
        hazard_rate(kn.t, g, kn.n, p, lambda, eta[b], 0, &h);
        const uint32_t lbits = st.status & (SBR_ODE_MAXITERS | SBR_STIFF_SWITCH | SBR_ODE_FAILED);
        for (int64_t j = 0; j < n_u; j++) {
            const int64_t o = b * n_u + j;
            point_t res;
            int64_t ns = 0;
            interest_point(kn.t, kn.x, kn.n, &h, t_end[b], u[j], kappa, r, delta, max_iters, rtol, atol, ode_maxiters,
                           &res, NULL, NULL, steps ? &ns : NULL, NULL);
            xi[o] = res.xi; tin[o] = res.tin; tout[o] = res.tout; aw_max[o] = res.aw_max; tol[o] = res.tol;
            status[o] = res.status | lbits;
            if (iters) iters[o] = res.iters;
            if (steps) steps[o] = ns;
        }
        hazard_free(&h);
        free(g);
        knots_free(&kn);
    }
    return rc;
}

/* one point with its paths (figure parity): res[5] = ξ, τ̄_IN, τ̄_OUT, AW_max, tol;
 * hr_tau / hr_v / V (n_hr each, caller-sized ≥ the learning knot count + 1) */
int64_t sbro_interest_point_opt(double beta, double eta, double t_end, double x0, double u, double p, double kappa,
                                double lambda, double r, double delta, double* res, uint32_t* status, double* hr_tau,
                                double* hr_v, double* V, double* aw, int64_t cap, int64_t* n_v, double rtol,
                                double atol, int64_t ode_maxiters)
{
    knots_t kn = {0};
    ode_stats_t st;
    ode_sys_t S;
    if (ode_solve(sys_logistic(&beta, &S), 1, 0.0, t_end, &x0, rtol, atol, ode_maxiters, &kn, &st)) return -1;
    double* g = (double*)malloc((size_t)kn.n * sizeof(double));
    for (int64_t i = 0; i < kn.n; i++) g[i] = (beta * kn.x[i]) * (1.0 - kn.x[i]);
    hazard_t h;
    hazard_rate(kn.t, g, kn.n, p, lambda, eta, 0, &h);
    int64_t nh = h.n;
    if (nh > cap) { hazard_free(&h); free(g); knots_free(&kn); return -nh; }
    point_t pr;
    interest_point(kn.t, kn.x, kn.n, &h, t_end, u, kappa, r, delta, 100, rtol, atol, ode_maxiters, &pr, V, n_v, NULL,
                   aw);
    if (aw && !(pr.status & SBR_RUN))
        for (int64_t i = 0; i < nh; i++) aw[i] = NAN;
    res[0] = pr.xi; res[1] = pr.tin; res[2] = pr.tout; res[3] = pr.aw_max; res[4] = pr.tol;
    *status = pr.status | (st.status & (SBR_ODE_MAXITERS | SBR_STIFF_SWITCH | SBR_ODE_FAILED));
    memcpy(hr_tau, h.tau, (size_t)nh * sizeof(double));
    memcpy(hr_v, h.hr, (size_t)nh * sizeof(double));
    hazard_free(&h);
    free(g);
    knots_free(&kn);
    return nh;
}

/* ------------------------------------------------------------------------ */
/* The entry points above under their earlier names and signatures, at the   */
/* reference's integrator options (reltol = abstol = eps(), maxiters = 1e6): */
/* a caller that binds them without the three trailing arguments gets what   */
/* it always got.                                                            */
/* ------------------------------------------------------------------------ */
#define SBRO_EPS 2.220446049250313e-16

int sbro_sweep_baseline(const double* beta, const double* eta, const double* t_end, double x0, const double* u,
                        int64_t n_beta, int64_t n_u, double p, double kappa, double lambda, int32_t max_iters,
                        int32_t nthreads, double* xi, double* tin, double* tout, double* aw_max, double* tol,
                        uint32_t* status, int32_t* iters, int64_t* nknots)
{
    return sbro_sweep_baseline_opt(beta, eta, t_end, x0, u, n_beta, n_u, p, kappa, lambda, max_iters, nthreads, xi, tin,
                                   tout, aw_max, tol, status, iters, nknots, SBRO_EPS, SBRO_EPS,
                                   SBR_DEFAULT_ODE_MAXITERS);
}

int64_t sbro_learn_hetero(const double* betas, const double* dist, int32_t K, double t1, double x0, double* t_out,
                          double* G_out, int64_t cap, int64_t* stats)
{
    return sbro_learn_hetero_opt(betas, dist, K, t1, x0, t_out, G_out, cap, stats, SBRO_EPS, SBRO_EPS,
                                 SBR_DEFAULT_ODE_MAXITERS);
}

int sbro_sweep_hetero(int32_t K, const double* betas, const double* dist, const double* eta, const double* t_end,
                      double x0, const double* u, int64_t n_col, int64_t n_u, double p, double kappa, double lambda,
                      int32_t max_iters, double tolerance, int32_t nthreads, double* xi, double* aw_max, double* tol,
                      uint32_t* status, int32_t* iters, double* tin_out, double* tout_out, int64_t* nknots)
{
    return sbro_sweep_hetero_opt(K, betas, dist, eta, t_end, x0, u, n_col, n_u, p, kappa, lambda, max_iters, tolerance,
                                 nthreads, xi, aw_max, tol, status, iters, tin_out, tout_out, nknots, SBRO_EPS,
                                 SBRO_EPS, SBR_DEFAULT_ODE_MAXITERS);
}

int64_t sbro_hetero_point_paths(int32_t K, const double* betas, const double* dist, double eta, double t_end,
                                double x0, double u, double p, double kappa, double lambda, double* res,
                                uint32_t* status, double* tin, double* tout, double* t_out, double* G_out,
                                double* aw_out, double* aw_groups, int64_t cap)
{
    return sbro_hetero_point_paths_opt(K, betas, dist, eta, t_end, x0, u, p, kappa, lambda, res, status, tin, tout,
                                       t_out, G_out, aw_out, aw_groups, cap, SBRO_EPS, SBRO_EPS,
                                       SBR_DEFAULT_ODE_MAXITERS);
}

int sbro_sweep_social(const double* beta, const double* eta, double x0, const double* u, int64_t n_beta, int64_t n_u,
                      double p, double kappa, double lambda, const double* cmp, int32_t n_cmp, double tol,
                      int32_t max_iter, int32_t bisect_max_iters, int32_t nthreads, double* xi, double* tin,
                      double* tout, double* aw_max, double* tl, uint32_t* status, int32_t* iters, int32_t* fp_iters,
                      int64_t* stats)
{
    return sbro_sweep_social_opt(beta, eta, x0, u, n_beta, n_u, p, kappa, lambda, cmp, n_cmp, tol, max_iter,
                                 bisect_max_iters, nthreads, xi, tin, tout, aw_max, tl, status, iters, fp_iters, stats,
                                 SBRO_EPS, SBRO_EPS, SBR_DEFAULT_ODE_MAXITERS);
}

int64_t sbro_social_point(double beta, double eta, double x0, double u, double p, double kappa, double lambda,
                          const double* cmp, int32_t n_cmp, double tol, int32_t max_iter, double* res,
                          uint32_t* status, int32_t* fp_iters, double* t_out, double* G_out, double* tau_out,
                          double* awo_out, int64_t cap, int64_t* n_tau)
{
    return sbro_social_point_opt(beta, eta, x0, u, p, kappa, lambda, cmp, n_cmp, tol, max_iter, res, status, fp_iters,
                                 t_out, G_out, tau_out, awo_out, cap, n_tau, SBRO_EPS, SBRO_EPS,
                                 SBR_DEFAULT_ODE_MAXITERS);
}

int sbro_sweep_interest(const double* beta, const double* eta, const double* t_end, double x0, const double* u,
                        int64_t n_beta, int64_t n_u, double p, double kappa, double lambda, double r, double delta,
                        int32_t max_iters, int32_t nthreads, double* xi, double* tin, double* tout, double* aw_max,
                        double* tol, uint32_t* status, int32_t* iters, int64_t* steps)
{
    return sbro_sweep_interest_opt(beta, eta, t_end, x0, u, n_beta, n_u, p, kappa, lambda, r, delta, max_iters,
                                   nthreads, xi, tin, tout, aw_max, tol, status, iters, steps, SBRO_EPS, SBRO_EPS,
                                   SBR_DEFAULT_ODE_MAXITERS);
}

int64_t sbro_interest_point(double beta, double eta, double t_end, double x0, double u, double p, double kappa,
                            double lambda, double r, double delta, double* res, uint32_t* status, double* hr_tau,
                            double* hr_v, double* V, double* aw, int64_t cap, int64_t* n_v)
{
    return sbro_interest_point_opt(beta, eta, t_end, x0, u, p, kappa, lambda, r, delta, res, status, hr_tau, hr_v, V,
                                   aw, cap, n_v, SBRO_EPS, SBRO_EPS, SBR_DEFAULT_ODE_MAXITERS);
}

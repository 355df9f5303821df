// MINPACK hybrj (Powell's hybrid dogleg with a user Jacobian) for the two-unknown TDoA system of
// multilateration.solve_trilateration_3d (multilateration.py:230-316), as scipy.optimize.fsolve runs it with
// fprime given: mode 1 (diagonal scaling from the Jacobian's column norms), factor 100, nprint 0.
// Restated from the published algorithm (Moré, Garbow, Hillstrom: User Guide for MINPACK-1, ANL-80-74,
// subroutines hybrj, qrfac, qform, dogleg, r1updt, r1mpyq, enorm), loop for loop and branch for branch, so
// that the iterates, the function-evaluation count and the termination code are the ones fsolve reports.
// Every comparison keeps the form of the original so that NaN inputs take the same branches.
// Header-only and __host__ __device__ so that the same code can be checked on a CPU build.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OFP_HYBRJ_HD __host__ __device__
#else
#define OFP_HYBRJ_HD
#endif

namespace ofp {
namespace hybrj {

constexpr int N = 2;             // unknowns (x, y) = equations
constexpr int LR = N * (N + 1) / 2;
constexpr double EPSMCH = 2.220446049250313e-16;   // dpmpar(1)
constexpr double GIANT = 1.7976931348623157e308;   // dpmpar(3)

// The residuals and Jacobian of multilateration.py:263-304: unknown point (x, y, 0), sensors o, a, b in 3-D.
struct Tdoa {
    double o[3], a[3], b[3];
    double dda, ddb;  // delta_d_a, delta_d_b

    OFP_HYBRJ_HD static double dist(double x, double y, const double* s) {
        const double dx = x - s[0], dy = y - s[1], dz = 0.0 - s[2];
        return sqrt(dx * dx + dy * dy + dz * dz);
    }
    OFP_HYBRJ_HD void f(const double* p, double* out) const {
        const double da = dist(p[0], p[1], a), db = dist(p[0], p[1], b), d0 = dist(p[0], p[1], o);
        out[0] = da - d0 - dda;
        out[1] = db - d0 - ddb;
    }
    // fj column-major, fj[i + N*j] = d f_i / d x_j
    OFP_HYBRJ_HD void jac(const double* p, double* fj) const {
        const double x = p[0], y = p[1];
        const double da = dist(x, y, a), db = dist(x, y, b), d0 = dist(x, y, o);
        fj[0 + N * 0] = (x - a[0]) / da - (x - o[0]) / d0;
        fj[0 + N * 1] = (y - a[1]) / da - (y - o[1]) / d0;
        fj[1 + N * 0] = (x - b[0]) / db - (x - o[0]) / d0;
        fj[1 + N * 1] = (y - b[1]) / db - (y - o[1]) / d0;
    }
};

OFP_HYBRJ_HD inline double enorm(int n, const double* x) {
    const double rdwarf = 3.834e-20, rgiant = 1.304e19;
    double s1 = 0, s2 = 0, s3 = 0, x1max = 0, x3max = 0;
    const double agiant = rgiant / (double)n;
    for (int i = 0; i < n; ++i) {
        const double xabs = fabs(x[i]);
        if (xabs > rdwarf && xabs < agiant) {
            s2 += xabs * xabs;
        } else if (xabs <= rdwarf) {
            if (xabs > x3max) {
                s3 = 1.0 + s3 * ((x3max / xabs) * (x3max / xabs));
                x3max = xabs;
            } else if (xabs != 0.0) {
                s3 += (xabs / x3max) * (xabs / x3max);
            }
        } else {
            if (xabs > x1max) {
                s1 = 1.0 + s1 * ((x1max / xabs) * (x1max / xabs));
                x1max = xabs;
            } else {
                s1 += (xabs / x1max) * (xabs / x1max);
            }
        }
    }
    if (s1 != 0.0) return x1max * sqrt(s1 + (s2 / x1max) / x1max);
    if (s2 != 0.0) {
        if (s2 >= x3max) return sqrt(s2 * (1.0 + (x3max / s2) * (x3max * s3)));
        return sqrt(x3max * ((s2 / x3max) + (x3max * s3)));
    }
    return x3max * sqrt(s3);
}

// qrfac without pivoting on the N x N column-major a: rdiag, acnorm (initial column norms)
OFP_HYBRJ_HD inline void qrfac(double* a, double* rdiag, double* acnorm) {
    for (int j = 0; j < N; ++j) {
        acnorm[j] = enorm(N, a + N * j);
        rdiag[j] = acnorm[j];
    }
    for (int j = 0; j < N; ++j) {
        double ajnorm = enorm(N - j, a + j + N * j);
        if (ajnorm != 0.0) {
            if (a[j + N * j] < 0.0) ajnorm = -ajnorm;
            for (int i = j; i < N; ++i) a[i + N * j] /= ajnorm;
            a[j + N * j] += 1.0;
            for (int k = j + 1; k < N; ++k) {
                double sum = 0.0;
                for (int i = j; i < N; ++i) sum += a[i + N * j] * a[i + N * k];
                const double temp = sum / a[j + N * j];
                for (int i = j; i < N; ++i) a[i + N * k] -= temp * a[i + N * j];
            }
        }
        rdiag[j] = -ajnorm;
    }
}

OFP_HYBRJ_HD inline void qform(double* q) {
    double wa[N];
    for (int j = 1; j < N; ++j)
        for (int i = 0; i < j; ++i) q[i + N * j] = 0.0;
    for (int l = 0; l < N; ++l) {
        const int k = N - 1 - l;
        for (int i = k; i < N; ++i) {
            wa[i] = q[i + N * k];
            q[i + N * k] = 0.0;
        }
        q[k + N * k] = 1.0;
        if (wa[k] == 0.0) continue;
        for (int j = k; j < N; ++j) {
            double sum = 0.0;
            for (int i = k; i < N; ++i) sum += q[i + N * j] * wa[i];
            const double temp = sum / wa[k];
            for (int i = k; i < N; ++i) q[i + N * j] -= temp * wa[i];
        }
    }
}

// r: upper triangle packed by rows (length LR)
OFP_HYBRJ_HD inline void dogleg(const double* r, const double* diag, const double* qtb, double delta, double* x) {
    double wa1[N], wa2[N];
    int jj = N * (N + 1) / 2;  // 0-based: index of r(jj) is jj - 1 in the loop below
    for (int k = 1; k <= N; ++k) {
        const int j = N - k;  // 0-based column
        jj -= k;              // 0-based index of the diagonal element of row j
        int l = jj + 1;
        double sum = 0.0;
        for (int i = j + 1; i < N; ++i) {
            sum += r[l] * x[i];
            ++l;
        }
        double temp = r[jj];
        if (temp == 0.0) {
            l = j;
            for (int i = 0; i <= j; ++i) {
                temp = fmax(temp, fabs(r[l]));
                l += N - 1 - i;
            }
            temp = EPSMCH * temp;
            if (temp == 0.0) temp = EPSMCH;
        }
        x[j] = (qtb[j] - sum) / temp;
    }
    for (int j = 0; j < N; ++j) {
        wa1[j] = 0.0;
        wa2[j] = diag[j] * x[j];
    }
    const double qnorm = enorm(N, wa2);
    if (qnorm <= delta) return;
    int l = 0;
    for (int j = 0; j < N; ++j) {
        const double temp = qtb[j];
        for (int i = j; i < N; ++i) {
            wa1[i] += r[l] * temp;
            ++l;
        }
        wa1[j] = wa1[j] / diag[j];
    }
    const double gnorm = enorm(N, wa1);
    double sgnorm = 0.0;
    double alpha = delta / qnorm;
    if (gnorm != 0.0) {
        for (int j = 0; j < N; ++j) wa1[j] = (wa1[j] / gnorm) / diag[j];
        l = 0;
        for (int j = 0; j < N; ++j) {
            double sum = 0.0;
            for (int i = j; i < N; ++i) {
                sum += r[l] * wa1[i];
                ++l;
            }
            wa2[j] = sum;
        }
        const double temp0 = enorm(N, wa2);
        sgnorm = (gnorm / temp0) / temp0;
        alpha = 0.0;
        if (!(sgnorm >= delta)) {
            const double bnorm = enorm(N, qtb);
            const double dq = delta / qnorm, sd = sgnorm / delta;
            double temp = (bnorm / gnorm) * (bnorm / qnorm) * sd;
            temp = temp - dq * (sd * sd) + sqrt((temp - dq) * (temp - dq) + (1.0 - dq * dq) * (1.0 - sd * sd));
            alpha = (dq * (1.0 - sd * sd)) / temp;
        }
    }
    const double temp = (1.0 - alpha) * fmin(sgnorm, delta);
    for (int j = 0; j < N; ++j) x[j] = temp * wa1[j] + alpha * x[j];
}

// r1updt with m = n = N; s packed by rows (length LR)
OFP_HYBRJ_HD inline bool r1updt(double* s, const double* u, double* v, double* w) {
    int jj = LR - 1;  // 0-based index of the last diagonal element
    w[N - 1] = s[jj];
    for (int nmj = 1; nmj <= N - 1; ++nmj) {
        const int j = N - 1 - nmj;
        jj -= N - j;
        w[j] = 0.0;
        if (v[j] == 0.0) continue;
        double sn, cs, tau;
        if (fabs(v[N - 1]) >= fabs(v[j])) {
            const double tn = v[j] / v[N - 1];
            cs = 0.5 / sqrt(0.25 + 0.25 * (tn * tn));
            sn = cs * tn;
            tau = sn;
        } else {
            const double ct = v[N - 1] / v[j];
            sn = 0.5 / sqrt(0.25 + 0.25 * (ct * ct));
            cs = sn * ct;
            tau = 1.0;
            if (fabs(cs) * GIANT > 1.0) tau = 1.0 / cs;
        }
        v[N - 1] = sn * v[j] + cs * v[N - 1];
        v[j] = tau;
        int l = jj;
        for (int i = j; i < N; ++i) {
            const double temp = cs * s[l] - sn * w[i];
            w[i] = sn * s[l] + cs * w[i];
            s[l] = temp;
            ++l;
        }
    }
    for (int i = 0; i < N; ++i) w[i] += v[N - 1] * u[i];
    bool sing = false;
    for (int j = 0; j < N - 1; ++j) {
        if (w[j] != 0.0) {
            double sn, cs, tau;
            if (fabs(s[jj]) >= fabs(w[j])) {
                const double tn = w[j] / s[jj];
                cs = 0.5 / sqrt(0.25 + 0.25 * (tn * tn));
                sn = cs * tn;
                tau = sn;
            } else {
                const double ct = s[jj] / w[j];
                sn = 0.5 / sqrt(0.25 + 0.25 * (ct * ct));
                cs = sn * ct;
                tau = 1.0;
                if (fabs(cs) * GIANT > 1.0) tau = 1.0 / cs;
            }
            int l = jj;
            for (int i = j; i < N; ++i) {
                const double temp = cs * s[l] + sn * w[i];
                w[i] = -sn * s[l] + cs * w[i];
                s[l] = temp;
                ++l;
            }
            w[j] = tau;
        }
        if (s[jj] == 0.0) sing = true;
        jj += N - j;
    }
    s[jj] = w[N - 1];
    if (s[jj] == 0.0) sing = true;
    return sing;
}

// r1mpyq: a (m x N, column-major with leading dimension lda) times the rotations in v, w
OFP_HYBRJ_HD inline void r1mpyq(int m, double* a, int lda, const double* v, const double* w) {
    double cs = 0.0, sn = 0.0;  // a NaN rotation keeps the previous one, as in the original
    for (int nmj = 1; nmj <= N - 1; ++nmj) {
        const int j = N - 1 - nmj;
        if (fabs(v[j]) > 1.0) cs = 1.0 / v[j];
        if (fabs(v[j]) > 1.0) sn = sqrt(1.0 - cs * cs);
        if (fabs(v[j]) <= 1.0) sn = v[j];
        if (fabs(v[j]) <= 1.0) cs = sqrt(1.0 - sn * sn);
        for (int i = 0; i < m; ++i) {
            const double temp = cs * a[i + lda * j] - sn * a[i + lda * (N - 1)];
            a[i + lda * (N - 1)] = sn * a[i + lda * j] + cs * a[i + lda * (N - 1)];
            a[i + lda * j] = temp;
        }
    }
    for (int j = 0; j < N - 1; ++j) {
        if (fabs(w[j]) > 1.0) cs = 1.0 / w[j];
        if (fabs(w[j]) > 1.0) sn = sqrt(1.0 - cs * cs);
        if (fabs(w[j]) <= 1.0) sn = w[j];
        if (fabs(w[j]) <= 1.0) cs = sqrt(1.0 - sn * sn);
        for (int i = 0; i < m; ++i) {
            const double temp = cs * a[i + lda * j] + sn * a[i + lda * (N - 1)];
            a[i + lda * (N - 1)] = -sn * a[i + lda * j] + cs * a[i + lda * (N - 1)];
            a[i + lda * j] = temp;
        }
    }
}

struct Result {
    double x[N];
    int info;  // fsolve's ier: 1 converged, 2 maxfev reached, 3 xtol too small, 4 / 5 not making progress
    int nfev;
};

// hybrj(fcn, n=2, x, xtol, maxfev, mode=1, factor) from the starting point x0
OFP_HYBRJ_HD inline Result solve(const Tdoa& fn, const double* x0, double xtol, int maxfev, double factor = 100.0) {
    const double p1 = 0.1, p5 = 0.5, p001 = 0.001, p0001 = 0.0001;
    Result res;
    double x[N], fvec[N], fjac[N * N], diag[N], r[LR], qtf[N], wa1[N], wa2[N], wa3[N], wa4[N];
    for (int j = 0; j < N; ++j) x[j] = x0[j];
    int info = 0, nfev = 0;
    if (!(xtol >= 0.0) || maxfev <= 0 || !(factor > 0.0)) {
        for (int j = 0; j < N; ++j) res.x[j] = x[j];
        res.info = 0;
        res.nfev = 0;
        return res;
    }
    fn.f(x, fvec);
    nfev = 1;
    double fnorm = enorm(N, fvec);
    double xnorm = 0.0, delta = 0.0;
    int iter = 1, ncsuc = 0, ncfail = 0, nslow1 = 0, nslow2 = 0;
    while (info == 0) {  // outer loop: a fresh Jacobian
        bool jeval = true;
        fn.jac(x, fjac);
        qrfac(fjac, wa1, wa2);
        if (iter == 1) {
            for (int j = 0; j < N; ++j) {
                diag[j] = wa2[j];
                if (wa2[j] == 0.0) diag[j] = 1.0;
            }
            for (int j = 0; j < N; ++j) wa3[j] = diag[j] * x[j];
            xnorm = enorm(N, wa3);
            delta = factor * xnorm;
            if (delta == 0.0) delta = factor;
        }
        for (int i = 0; i < N; ++i) qtf[i] = fvec[i];
        for (int j = 0; j < N; ++j) {
            if (fjac[j + N * j] != 0.0) {
                double sum = 0.0;
                for (int i = j; i < N; ++i) sum += fjac[i + N * j] * qtf[i];
                const double temp = -sum / fjac[j + N * j];
                for (int i = j; i < N; ++i) qtf[i] += fjac[i + N * j] * temp;
            }
        }
        for (int j = 0; j < N; ++j) {
            int l = j;
            for (int i = 0; i < j; ++i) {
                r[l] = fjac[i + N * j];
                l += N - 1 - i;
            }
            r[l] = wa1[j];
        }
        qform(fjac);
        for (int j = 0; j < N; ++j) diag[j] = fmax(diag[j], wa2[j]);
        while (true) {  // inner loop
            dogleg(r, diag, qtf, delta, wa1);
            for (int j = 0; j < N; ++j) {
                wa1[j] = -wa1[j];
                wa2[j] = x[j] + wa1[j];
                wa3[j] = diag[j] * wa1[j];
            }
            const double pnorm = enorm(N, wa3);
            if (iter == 1) delta = fmin(delta, pnorm);
            fn.f(wa2, wa4);
            nfev += 1;
            const double fnorm1 = enorm(N, wa4);
            double actred = -1.0;
            if (fnorm1 < fnorm) actred = 1.0 - (fnorm1 / fnorm) * (fnorm1 / fnorm);
            int l = 0;
            for (int i = 0; i < N; ++i) {
                double sum = 0.0;
                for (int j = i; j < N; ++j) {
                    sum += r[l] * wa1[j];
                    ++l;
                }
                wa3[i] = qtf[i] + sum;
            }
            const double temp = enorm(N, wa3);
            double prered = 0.0;
            if (temp < fnorm) prered = 1.0 - (temp / fnorm) * (temp / fnorm);
            double ratio = 0.0;
            if (prered > 0.0) ratio = actred / prered;
            if (!(ratio >= p1)) {
                ncsuc = 0;
                ncfail += 1;
                delta = p5 * delta;
            } else {
                ncfail = 0;
                ncsuc += 1;
                if (ratio >= p5 || ncsuc > 1) delta = fmax(delta, pnorm / p5);
                if (fabs(ratio - 1.0) <= p1) delta = pnorm / p5;
            }
            if (!(ratio < p0001)) {
                for (int j = 0; j < N; ++j) {
                    x[j] = wa2[j];
                    wa2[j] = diag[j] * x[j];
                    fvec[j] = wa4[j];
                }
                xnorm = enorm(N, wa2);
                fnorm = fnorm1;
                iter += 1;
            }
            nslow1 += 1;
            if (actred >= p001) nslow1 = 0;
            if (jeval) nslow2 += 1;
            if (actred >= p1) nslow2 = 0;
            if (delta <= xtol * xnorm || fnorm == 0.0) info = 1;
            if (info != 0) break;
            if (nfev >= maxfev) info = 2;
            if (p1 * fmax(p1 * delta, pnorm) <= EPSMCH * xnorm) info = 3;
            if (nslow2 == 5) info = 4;
            if (nslow1 == 10) info = 5;
            if (info != 0) break;
            if (ncfail == 2) break;  // recompute the Jacobian
            for (int j = 0; j < N; ++j) {
                double sum = 0.0;
                for (int i = 0; i < N; ++i) sum += fjac[i + N * j] * wa4[i];
                wa2[j] = (sum - wa3[j]) / pnorm;
                wa1[j] = diag[j] * ((diag[j] * wa1[j]) / pnorm);
                if (ratio >= p0001) qtf[j] = sum;
            }
            r1updt(r, wa1, wa2, wa3);
            r1mpyq(N, fjac, N, wa2, wa3);
            r1mpyq(1, qtf, 1, wa2, wa3);
            jeval = false;
        }
    }
    for (int j = 0; j < N; ++j) res.x[j] = x[j];
    res.info = info;
    res.nfev = nfev;
    return res;
}

}  // namespace hybrj
}  // namespace ofp

// More-Thuente line search (More & Thuente 1994) with the safeguards of the reference's library (lbfgs/lib/lbfgs.cpp:815-1004,
// :1128-1295): the one copy that the plmDCA and the arDCA optimisers run.  Host code only, scalars in double, no HIP header:
// a host compiler builds it, and tests/test_more_thuente_host.py holds it against the oracle's C restatement step for step.
#pragma once

#include <algorithm>
#include <cmath>

// libLBFGS status codes (lbfgs/include/lbfgs.h:76-149)
enum {
    LB_OUTOFINTERVAL = -1003, LB_INCORRECT_TMINMAX = -1002, LB_ROUNDING_ERROR = -1001, LB_MINIMUMSTEP = -1000,
    LB_MAXIMUMSTEP = -999, LB_MAXIMUMLINESEARCH = -998, LB_MAXIMUMITERATION = -997, LB_WIDTHTOOSMALL = -996,
    LB_INVALIDPARAMETERS = -995, LB_INCREASEGRADIENT = -994, LB_ALREADY_MINIMIZED = 2
};

struct LsPoint { double st, f, d; };

inline double cubic_min(double u, double fu, double du, double v, double fv, double dv)
{
    const double d = v - u;
    const double theta = (fu - fv) * 3 / d + du + dv;
    const double s = std::max(std::fabs(theta), std::max(std::fabs(du), std::fabs(dv)));
    const double a = theta / s;
    double gamma = s * std::sqrt(a * a - (du / s) * (dv / s));
    if (v < u) gamma = -gamma;
    const double p = gamma - du + theta, q = gamma - du + gamma + dv;
    return u + (p / q) * d;
}
inline double cubic_min_clamped(double u, double fu, double du, double v, double fv, double dv, double lo, double hi)
{
    const double d = v - u;
    const double theta = (fu - fv) * 3 / d + du + dv;
    const double s = std::max(std::fabs(theta), std::max(std::fabs(du), std::fabs(dv)));
    const double a = theta / s;
    double gamma = s * std::sqrt(std::max(0.0, a * a - (du / s) * (dv / s)));
    if (u < v) gamma = -gamma;
    const double p = gamma - dv + theta, q = gamma - dv + gamma + du;
    const double r = p / q;
    if (r < 0. && gamma != 0.) return v - r * d;
    return a < 0 ? hi : lo;
}
inline double quad_min_f(double u, double fu, double du, double v, double fv)
{
    const double a = v - u;
    return u + du / ((fu - fv) / a + du) / 2 * a;
}
inline double quad_min_d(double u, double du, double v, double dv)
{
    const double a = u - v;
    return v + dv / (dv - du) * a;
}

// Trial-interval update: best / other are the end points of the interval, t / ft / dt the trial (t receives the next one).
// 0, or the LB_* code of a trial outside the interval or an end point that is no descent.
inline int mt_update(LsPoint& best, LsPoint& other, double& t, double ft, double dt, double tmin, double tmax, bool& brackt)
{
    const bool opposite = (dt * (best.d / std::fabs(best.d)) < 0.);
    bool bound;
    double newt;
    if (brackt) {
        if (t <= std::min(best.st, other.st) || std::max(best.st, other.st) <= t) return LB_OUTOFINTERVAL;
        if (0. <= best.d * (t - best.st)) return LB_INCREASEGRADIENT;
        if (tmax < tmin) return LB_INCORRECT_TMINMAX;
    }
    if (best.f < ft) {
        brackt = true; bound = true;
        const double mc = cubic_min(best.st, best.f, best.d, t, ft, dt);
        const double mq = quad_min_f(best.st, best.f, best.d, t, ft);
        newt = (std::fabs(mc - best.st) < std::fabs(mq - best.st)) ? mc : mc + 0.5 * (mq - mc);
    } else if (opposite) {
        brackt = true; bound = false;
        const double mc = cubic_min(best.st, best.f, best.d, t, ft, dt);
        const double mq = quad_min_d(best.st, best.d, t, dt);
        newt = (std::fabs(mc - t) > std::fabs(mq - t)) ? mc : mq;
    } else if (std::fabs(dt) < std::fabs(best.d)) {
        bound = true;
        const double mc = cubic_min_clamped(best.st, best.f, best.d, t, ft, dt, tmin, tmax);
        const double mq = quad_min_d(best.st, best.d, t, dt);
        if (brackt) newt = (std::fabs(t - mc) < std::fabs(t - mq)) ? mc : mq;
        else newt = (std::fabs(t - mc) > std::fabs(t - mq)) ? mc : mq;
    } else {
        bound = false;
        if (brackt) newt = cubic_min(t, ft, dt, other.st, other.f, other.d);
        else newt = (best.st < t) ? tmax : tmin;
    }
    if (best.f < ft) {
        other = LsPoint{t, ft, dt};
    } else {
        if (opposite) other = best;
        best = LsPoint{t, ft, dt};
    }
    newt = std::min(newt, tmax);
    newt = std::max(newt, tmin);
    if (brackt && bound) {
        const double mq = best.st + 0.66 * (other.st - best.st);
        if (best.st < other.st) newt = std::min(newt, mq);
        else newt = std::max(newt, mq);
    }
    t = newt;
    return 0;
}

struct MtParams { double ftol, gtol, xtol, min_step, max_step; int max_ls; };

// The search from a point with value *f along a direction (lbfgs.cpp:815-1004).  eval(stp, &f, &dg) moves to step stp,
// evaluates there and yields the value and g.d; what it returns other than 0 is a runtime error: it ends the search, goes
// to *rc, and the result is 0.  Otherwise the result is the number of evaluations (> 0, *stp and *f those of the accepted
// point) or an LB_* code.
// *dginit is g.d at the starting point.  With slope_deferred it is not known yet and the first eval() writes it (nothing
// before that evaluation depends on it); a direction found then to be no descent gives LB_INCREASEGRADIENT with *f
// restored, where the reference returns before it evaluates (lbfgs.cpp:858-861).
template <typename Eval>
int mt_line_search(const MtParams& p, double* stp, double* f, const double* dginit, bool slope_deferred, Eval&& eval, int* rc)
{
    int count = 0, uinfo = 0;
    bool brackt = false, stage1 = true;
    *rc = 0;
    if (*stp <= 0.) return LB_INVALIDPARAMETERS;
    if (!slope_deferred && 0 < *dginit) return LB_INCREASEGRADIENT;
    const double finit = *f;
    double dg0 = slope_deferred ? 0. : *dginit;
    double dgtest = p.ftol * dg0;
    double width = p.max_step - p.min_step, prev_width = 2.0 * width;
    LsPoint bx{0., finit, dg0}, by{0., finit, dg0};
    for (;;) {
        double stmin, stmax;
        if (brackt) { stmin = std::min(bx.st, by.st); stmax = std::max(bx.st, by.st); }
        else { stmin = bx.st; stmax = *stp + 4.0 * (*stp - bx.st); }
        if (*stp < p.min_step) *stp = p.min_step;
        if (p.max_step < *stp) *stp = p.max_step;
        if ((brackt && ((*stp <= stmin || stmax <= *stp) || p.max_ls <= count + 1 || uinfo != 0)) ||
            (brackt && (stmax - stmin <= p.xtol * stmax)))
            *stp = bx.st;
        double dg;
        if ((*rc = eval(*stp, f, &dg))) return 0;
        if (slope_deferred && count == 0) {
            dg0 = *dginit;
            if (0 < dg0) { *f = finit; return LB_INCREASEGRADIENT; }
            dgtest = p.ftol * dg0;
            bx.d = by.d = dg0;
        }
        const double ftest1 = finit + *stp * dgtest;
        ++count;
        if (brackt && ((*stp <= stmin || stmax <= *stp) || uinfo != 0)) return LB_ROUNDING_ERROR;
        if (*stp == p.max_step && *f <= ftest1 && dg <= dgtest) return LB_MAXIMUMSTEP;
        if (*stp == p.min_step && (ftest1 < *f || dgtest <= dg)) return LB_MINIMUMSTEP;
        if (brackt && (stmax - stmin) <= p.xtol * stmax) return LB_WIDTHTOOSMALL;
        if (p.max_ls <= count) return LB_MAXIMUMLINESEARCH;
        if (*f <= ftest1 && std::fabs(dg) <= p.gtol * (-dg0)) return count;      // strong Wolfe conditions
        if (stage1 && *f <= ftest1 && std::min(p.ftol, p.gtol) * dg0 <= dg) stage1 = false;
        if (stage1 && ftest1 < *f && *f <= bx.f) {
            // stage 1 works on the modified function psi(t) = f(t) - f(0) - ftol t f'(0)
            LsPoint mx{bx.st, bx.f - bx.st * dgtest, bx.d - dgtest};
            LsPoint my{by.st, by.f - by.st * dgtest, by.d - dgtest};
            uinfo = mt_update(mx, my, *stp, *f - *stp * dgtest, dg - dgtest, stmin, stmax, brackt);
            bx = LsPoint{mx.st, mx.f + mx.st * dgtest, mx.d + dgtest};
            by = LsPoint{my.st, my.f + my.st * dgtest, my.d + dgtest};
        } else {
            uinfo = mt_update(bx, by, *stp, *f, dg, stmin, stmax, brackt);
        }
        if (brackt) {
            if (0.66 * prev_width <= std::fabs(by.st - bx.st)) *stp = bx.st + 0.5 * (by.st - bx.st);
            prev_width = width;
            width = std::fabs(by.st - bx.st);
        }
    }
}

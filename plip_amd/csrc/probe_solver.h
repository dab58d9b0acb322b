// probe_solver.h -- host side of plipmi_probe_fit: one L-BFGS state machine per one-vs-rest problem.
//
// The K problems are separable, so each keeps its own memory (10 pairs), direction and line search, all in double; what they share
// is the evaluation: every pass of probe_loss_grad_kernel evaluates all K current trial points at once.  A problem is fed the
// loss and gradient at its trial point and answers with its next one (a shorter step along the same direction, or a step along a
// new direction); a problem that has finished keeps handing out its final point.
// plipmi_softmax_fit runs ONE such machine over all C (D + 1) variables: a softmax couples the classes (probe_softmax.hip).
//
// Line search: backtracking from the unit step (first iteration: 1 / |g|), the next trial from the secant of the directional
// derivative.  A step is accepted on the Armijo condition, or -- close to the minimum, where differences of f drown in the
// fp32 rounding of its terms while the gradient is still accurate -- on the approximate Wolfe conditions of Hager & Zhang
// (SIAM J. Optim. 16, 2005): f not larger than f(0) (1 + 1e-6) and  0.9 phi'(0) <= phi'(step) <= -0.8 phi'(0).
// The trial points are rounded to fp32 (what the kernel reads) BEFORE the step and gradient differences are formed, so the
// curvature pairs describe the points that were really evaluated.
#pragma once
#include <math.h>

#include <vector>

namespace plipmi {

struct ProbeLbfgs {
  static constexpr int kMem = 10, kMaxTries = 40;
  int n = 0, max_iter = 0;
  double gtol = 0;
  std::vector<double> x, g, dir, xt;
  std::vector<std::vector<double>> S, Y;
  std::vector<double> rho;
  double f = 0, gd = 0, step = 0, gnorm = 0;
  int iters = 0, tries = 0;
  bool started = false, done = false, converged = false;

  void init(const float* x0, int n_, int max_iter_, double gtol_) {
    n = n_; max_iter = max_iter_; gtol = gtol_;
    x.assign(n, 0); g.assign(n, 0); dir.assign(n, 0);
    xt.assign(x0, x0 + n);
  }
  void trial(float* out) const { for (int i = 0; i < n; ++i) out[i] = (float)xt[i]; }

  static double dot(const std::vector<double>& a, const std::vector<double>& b) {
    double s = 0;
    for (size_t i = 0; i < a.size(); ++i) s += a[i] * b[i];
    return s;
  }
  void set_trial() {
    for (int i = 0; i < n; ++i) xt[i] = (double)(float)(x[i] + step * dir[i]);
  }
  void finish(bool ok) { done = true; converged = ok; xt = x; }
  void accept(double ft, const std::vector<double>& gt) {
    x = xt; f = ft; g = gt;
    gnorm = 0;
    for (double v : g) gnorm = fmax(gnorm, fabs(v));
  }
  void new_direction() {
    // two-loop recursion
    const int m = (int)S.size();
    std::vector<double> q = g, a(m);
    for (int i = m - 1; i >= 0; --i) {
      a[i] = rho[i] * dot(S[i], q);
      for (int j = 0; j < n; ++j) q[j] -= a[i] * Y[i][j];
    }
    if (m) {
      const double gamma = dot(S[m - 1], Y[m - 1]) / dot(Y[m - 1], Y[m - 1]);
      for (double& v : q) v *= gamma;
    }
    for (int i = 0; i < m; ++i) {
      const double b = rho[i] * dot(Y[i], q);
      for (int j = 0; j < n; ++j) q[j] += (a[i] - b) * S[i][j];
    }
    for (int j = 0; j < n; ++j) dir[j] = -q[j];
    gd = dot(g, dir);
    if (!(gd < 0)) {                    // not a descent direction (rounding): restart from steepest descent
      S.clear(); Y.clear(); rho.clear();
      for (int j = 0; j < n; ++j) dir[j] = -g[j];
      gd = -dot(g, g);
    }
    step = S.empty() ? 1.0 / fmax(sqrt(-gd), 1e-300) : 1.0;
    tries = 0;
    set_trial();
  }

  // loss and gradient at the trial point
  void feed(double ft, const float* gt_f) {
    if (done) return;
    std::vector<double> gt(gt_f, gt_f + n);
    if (!started) {
      started = true;
      accept(ft, gt);
      if (gnorm <= gtol) return finish(true);
      return new_direction();
    }
    const double gdt = dot(gt, dir);
    const bool finite = isfinite(ft) && isfinite(gdt);
    const bool armijo = finite && ft <= f + 1e-4 * step * gd;
    const bool approx = finite && ft <= f + 1e-6 * fabs(f) && gdt >= 0.9 * gd && gdt <= -0.8 * gd;
    if (armijo || approx) {
      std::vector<double> s(n), yv(n);
      for (int j = 0; j < n; ++j) { s[j] = xt[j] - x[j]; yv[j] = gt[j] - g[j]; }
      accept(ft, gt);
      ++iters;
      if (gnorm <= gtol) return finish(true);
      if (iters >= max_iter) return finish(false);
      const double sy = dot(s, yv);
      if (sy > 1e-12 * sqrt(dot(s, s) * dot(yv, yv))) {
        if ((int)S.size() == kMem) { S.erase(S.begin()); Y.erase(Y.begin()); rho.erase(rho.begin()); }
        S.push_back(s); Y.push_back(yv); rho.push_back(1.0 / sy);
      }
      return new_direction();
    }
    if (++tries >= kMaxTries) return finish(false);
    // phi' is increasing (convex): the secant's zero of it, kept inside [0.1, 0.5] of the step
    double t = finite && gdt > gd ? -gd / (gdt - gd) : 0.5;
    step *= fmin(0.5, fmax(0.1, t));
    set_trial();
  }
};

}  // namespace plipmi

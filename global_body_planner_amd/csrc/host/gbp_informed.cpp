// gbp_informed.cpp — the ellipse of informed sampling (gbp.h
// gbp_informed_ellipse): one host statement, no engine call, compiled without
// FMA contraction so that every step below is its own binary64 rounding.
// tests/informed_ref.py restates it; tests/native/informed_probe.cpp runs it
// under sanitizers.
#include <cmath>

#include "gbp.h"

namespace {
constexpr double MY_PI = 3.14159;  // the planner's (gbp_closed_forms.h)
}

extern "C" __attribute__((visibility("default"))) int gbp_informed_ellipse(
    const double *focus_a, const double *focus_b, double cost, const double bounds[4],
    gbp_informed *out) {
  if (!focus_a || !focus_b || !bounds || !out) return GBP_E_INVALID_ARG;
  const double ax = focus_a[0], ay = focus_a[1], bx = focus_b[0], by = focus_b[1];
  if (std::isnan(ax) || std::isnan(ay) || std::isnan(bx) || std::isnan(by)) return GBP_E_INVALID_ARG;
  if (std::isnan(cost) || !(cost > 0)) return GBP_E_INVALID_ARG;
  const double dx = bx - ax, dy = by - ay;
  const double d = std::sqrt(dx * dx + dy * dy);
  gbp_informed e;
  e.reserved = 0;
  e.cost = cost;
  e.ux = d > 0 ? dx / d : 1;
  e.uy = d > 0 ? dy / d : 0;
  e.cx = (ax + bx) * 0.5;
  e.cy = (ay + by) * 0.5;
  e.a = cost * 0.5;
  const double w = cost * cost - d * d;
  e.b = w > 0 ? std::sqrt(w) * 0.5 : 0;
  e.active = cost < INFINITY &&
             (MY_PI * e.a) * e.b < (bounds[1] - bounds[0]) * (bounds[3] - bounds[2]);
  *out = e;
  return GBP_OK;
}

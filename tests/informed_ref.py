"""Informed sampling restated in numpy from the oracle's primitives (gbp.h
gbp_informed): the ellipse of two foci and a cost, and the draw
inside it.

Path cost is a sum of poseDistance (3-D) and a 2-D distance never exceeds it,
so a state on a path shorter than c between the trees' roots A and B satisfies
|p.xy - A.xy| + |p.xy - B.xy| < c: the ellipse in xy with those foci and major
axis c.  Every step below is one binary64 operation, as the product's build
(no FMA contraction) makes it; the uniforms are orc_uniform2's, log and sincos
oracle.rmath's, the height orc_ground_height's, and q[3..7] are the oracle's
plain draw of the same index.
"""
import ctypes

import numpy as np

import oracle

MY_PI = 3.14159          # the planner's (planning_utils.h)
H_MIN, H_MAX, ROBOT_H = 0.075, 0.4, 0.05
PURPOSE_STATE = 1

# the session tests' search: synth-rough-256, 5.1 m x 5.1 m
SESSION_START = (1.0, 2.55)
SESSION_GOAL = (4.02, 2.55)

FIELDS = ("cost", "cx", "cy", "ux", "uy", "a", "b")


def ellipse(focus_a, focus_b, cost, bounds):
    """gbp_informed_ellipse: a dict of the record's fields, or None where the
    entry refuses (a NaN focus coordinate, a NaN cost, cost <= 0)."""
    f = np.float64
    ax, ay, bx, by = f(focus_a[0]), f(focus_a[1]), f(focus_b[0]), f(focus_b[1])
    cost = f(cost)
    if np.isnan([ax, ay, bx, by, cost]).any() or not cost > 0:
        return None
    with np.errstate(all="ignore"):
        dx = bx - ax
        dy = by - ay
        d = np.sqrt(dx * dx + dy * dy)
        ux = dx / d if d > 0 else f(1)
        uy = dy / d if d > 0 else f(0)
        cx = (ax + bx) * f(0.5)
        cy = (ay + by) * f(0.5)
        a = cost * f(0.5)
        w = cost * cost - d * d
        b = np.sqrt(w) * f(0.5) if w > 0 else f(0)
        area = (f(MY_PI) * a) * b
        box = (f(bounds[1]) - f(bounds[0])) * (f(bounds[3]) - f(bounds[2]))
    return {"active": int(bool(cost < np.inf and area < box)), "cost": cost, "cx": cx, "cy": cy,
            "ux": ux, "uy": uy, "a": a, "b": b}


def uniforms(n, seed, stream_id, index_base, draw):
    """orc_uniform2(seed, stream, PURPOSE_STATE, index_base + i, draw) for i < n: [n][2]"""
    f = oracle.lib().orc_uniform2
    out = np.empty((n, 2))
    u = (ctypes.c_double * 2)()
    for i in range(n):
        f(seed, stream_id, PURPOSE_STATE, index_base + i, draw, u)
        out[i, 0], out[i, 1] = u[0], u[1]
    return out


def draws(O, e, n, seed, stream_id, index_base=0):
    """Try 0 of indices index_base .. index_base + n - 1 under the ellipse e (a
    dict as ellipse() returns): [n][8].  e["active"] == 0: the plain draws."""
    plain, _ = O.sample_states(n, seed, stream_id, index_base, nthreads=8)
    if not e["active"]:
        return plain
    f = np.float64
    u0 = uniforms(n, seed, stream_id, index_base, 0)
    u1 = uniforms(n, seed, stream_id, index_base, 1)
    q = plain.copy()
    r = np.sqrt(u0[:, 0])
    th = (2.0 * MY_PI) * u0[:, 1]
    sc = oracle.rmath(1, th)
    si, co = sc[:, 0], sc[:, 1]
    ex = (f(e["a"]) * r) * co
    ey = (f(e["b"]) * r) * si
    q[:, 0] = f(e["cx"]) + (f(e["ux"]) * ex - f(e["uy"]) * ey)
    q[:, 1] = f(e["cy"]) + (f(e["uy"]) * ex + f(e["ux"]) * ey)
    # the clipped Gaussian above the ground (planner_class.cpp:44-58); box_muller's z0
    z_min_rel, z_max_rel = H_MIN + ROBOT_H, H_MAX + ROBOT_H
    mean = 0.5 * (z_max_rel + z_min_rel)
    sd = (z_max_rel - z_min_rel) * (1.0 / (2 * 3.0))
    rr = np.sqrt(-2.0 * oracle.rmath(0, 1.0 - u1[:, 0]))
    z0 = rr * oracle.rmath(1, 6.283185307179586 * u1[:, 1])[:, 1]
    hz = z0 * sd + mean
    rel = np.where(hz < z_max_rel, hz, z_max_rel)       # std::min(hz, z_max_rel)
    rel = np.where(rel < z_min_rel, z_min_rel, rel)     # std::max(., z_min_rel)
    g = np.array([O.ground_height(float(x), float(y))[0] for x, y in q[:, :2]])  # NaN off the map
    q[:, 2] = rel + g
    return q

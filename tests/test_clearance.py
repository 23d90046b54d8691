"""Clearance report (agx_ocp_clearance, DESIGN.md section 4 "Diagnostics"): the numpy distance reference of the GPU tests in
tests/test_clearance_gpu.py, pinned here to the CPU checker, and the argument checks of `HipOcp.clearance`.

The reference is closed forms on top of the forward kinematics of tests/joint_ref.py (chains, trees, prismatic joints):
sphere / sphere, sphere / capsule and capsule / capsule as point / point, point / segment and segment / segment distances minus
the radii, and the distance of a point to the SURFACE of a sphere, a capsule or a box for the witness points.  The segment /
segment distance is written as the smallest of the interior stationary point and the four end-point-to-segment distances, not
as the clamped sequence of the device routine.  The box pairs of the 64-pair chain case have the checker as their reference.

Box against capsule or sphere and the degenerate capsule pairs (parallel, nearly parallel, collinear, crossing axes) have an exact
reference of their own further down, on world-fixed frames and in numpy longdouble: `degenerate_scene` and `exact_distance`.
"""
import ctypes as C

import numpy as np
import pytest

import joint_ref as jr
from agimus_controller_amd import _abi, workloads
from agimus_controller_amd.factory import robot_tables as rt

B = 3
CAPS = [f"cap{j}" for j in range(1, 6)]
SELF = [("cap1", "cap3"), ("cap1", "cap4"), ("cap1", "cap5"), ("cap2", "cap5")]


def _chain():
    """The table of tests/test_many_collision_costs.py::_chain, rebuilt: chain_table(6, seed=3) with a capsule (r 0.04, half length
    0.06) on joints 1 .. 5 and twelve seeded world capsules, spheres and boxes."""
    t = rt.chain_table(6, seed=3)
    for j in range(1, 6):
        t = t.with_geometry(f"cap{j}", j, rt.se3(None, [0.0, 0.0, 0.05]), 0.04, 0.06)
    rng = np.random.default_rng(5)
    for i in range(12):
        d = rng.normal(size=3)
        xyz = list(rng.uniform(0.45, 0.9) * d / np.linalg.norm(d))
        if i % 3 == 0:
            t = t.with_geometry(f"ob{i}", -1, rt.se3(rt.rpy(0.0, np.pi / 2, 0.0), xyz), rng.uniform(0.03, 0.07), rng.uniform(0.05, 0.15))
        elif i % 3 == 1:
            t = t.with_geometry(f"ob{i}", -1, rt.se3(None, xyz), rng.uniform(0.03, 0.07), 0.0)
        else:
            t = t.with_geometry(f"ob{i}", -1, rt.se3(None, xyz), box=tuple(rng.uniform(0.03, 0.08, 3)))
    return t


def _pairs(n):
    """n pairs: the four self pairs first, then link capsule x obstacle (as _pairs of that file)."""
    world = [(c, f"ob{i}") for i in range(12) for c in CAPS]
    out = (SELF + world)[:n]
    assert len(out) == n
    return out


# ------------------------------------------------------------------------------------------------------ numpy reference
def is_box(t, f):
    return t.frame_box is not None and bool(np.any(np.asarray(t.frame_box, dtype=float).reshape(-1, 3)[f] > 0.0))


def geometry(t, f, q):
    """(R [..., 3, 3], p [..., 3], radius, half length, box half extents or None) of geometry frame f at q [..., nv]."""
    R, p = jr.frame_placement(t, f, np.asarray(q, dtype=float))
    hl = 0.0 if t.frame_halflen is None else float(t.frame_halflen[f])
    box = np.asarray(t.frame_box, dtype=float).reshape(-1, 3)[f] if is_box(t, f) else None
    return R, p, float(t.frame_radius[f]), hl, box


def point_segment(x, a0, a1):
    """Distance of the points x [..., 3] to the segments a0 a1 [..., 3] (a0 == a1: a point)."""
    d = a1 - a0
    dd = (d * d).sum(-1)
    s = np.clip(((x - a0) * d).sum(-1) / np.where(dd > 0.0, dd, 1.0), 0.0, 1.0)
    e = x - (a0 + s[..., None] * d)
    return np.sqrt((e * e).sum(-1))


def segment_segment(a0, a1, b0, b1):
    """Distance of the segments a0 a1 and b0 b1 [..., 3], both of positive length: the stationary point of the two lines where it
    lies inside both segments, otherwise the smallest of the four end-point-to-segment distances."""
    d1, d2, r = a1 - a0, b1 - b0, a0 - b0
    a, e, b = (d1 * d1).sum(-1), (d2 * d2).sum(-1), (d1 * d2).sum(-1)
    c, f = (d1 * r).sum(-1), (d2 * r).sum(-1)
    den = a * e - b * b
    ok = den > 1e-12 * a * e
    safe = np.where(ok, den, 1.0)
    s, t = (b * f - c * e) / safe, (a * f - b * c) / safe
    inside = ok & (s >= 0.0) & (s <= 1.0) & (t >= 0.0) & (t <= 1.0)
    g = (a0 + s[..., None] * d1) - (b0 + t[..., None] * d2)
    ends = np.minimum(np.minimum(point_segment(a0, b0, b1), point_segment(a1, b0, b1)), np.minimum(point_segment(b0, a0, a1), point_segment(b1, a0, a1)))
    return np.where(inside, np.sqrt((g * g).sum(-1)), ends)


def _ends(R, p, hl):
    z = R[..., :, 2]
    return p - hl * z, p + hl * z


def distance(t, fa, fb, q):
    """Signed distance [...] of the sphere / capsule pair (fa, fb) at q [..., nv] (negative: the overlap of two spheres or capsules)."""
    Ra, pa, ra, ha, ba = geometry(t, fa, q)
    Rb, pb, rb, hb, bb = geometry(t, fb, q)
    assert ba is None and bb is None, "box pairs have no closed form here"
    if ha == 0.0 and hb == 0.0:
        e = pa - pb
        d = np.sqrt((e * e).sum(-1))
    elif ha == 0.0:
        d = point_segment(pa, *_ends(Rb, pb, hb))
    elif hb == 0.0:
        d = point_segment(pb, *_ends(Ra, pa, ha))
    else:
        d = segment_segment(*_ends(Ra, pa, ha), *_ends(Rb, pb, hb))
    return d - (ra + rb)


def surface_distance(t, f, q, x):
    """|distance| of the world points x [..., 3] to the surface of geometry f at q [..., nv]: sphere, capsule or box."""
    R, p, r, hl, box = geometry(t, f, q)
    if box is None:
        return np.abs(point_segment(x, *_ends(R, p, hl)) - r)
    xl = (np.swapaxes(R, -1, -2) @ (x - p)[..., None])[..., 0]
    out = np.maximum(np.abs(xl) - box, 0.0)
    outside = np.sqrt((out * out).sum(-1))
    return np.where(outside > 0.0, outside, (box - np.abs(xl)).min(-1))


def reference(t, pairs, q):
    """dist [..., n] of the pairs (frame ids or names) at q [..., nv]; every pair a sphere / capsule pair."""
    ids = [(t.frame_id(a), t.frame_id(b)) for a, b in pairs]
    return np.stack([distance(t, a, b, q) for a, b in ids], -1)


# ------------------------------------------------------------------------------- exact references on world-fixed frames
LD = np.longdouble


def segment_box(e0, e1, half):
    """Distance of the segment e0 e1 (box frame; e0 == e1: a point) to the box [-half, half], 0 when they meet.  Along the segment
    dist^2 = sum_k max(|x_k| - half_k, 0)^2 is piecewise quadratic with breakpoints where a coordinate meets +- half_k: the
    smallest of its values at the breakpoints, at the ends and at the clamped minimiser of every piece."""
    e0, e1, half = (np.asarray(v, dtype=LD) for v in (e0, e1, half))
    d = e1 - e0

    def f2(s):
        o = np.maximum(np.abs(e0 + s * d) - half, LD(0))
        return (o * o).sum()

    cuts = {LD(0), LD(1)}
    for k in range(3):
        for sg in (-1, 1):
            if d[k] != 0 and 0 < (sg * half[k] - e0[k]) / d[k] < 1:
                cuts.add((sg * half[k] - e0[k]) / d[k])
    cuts = sorted(cuts)
    best = min(f2(s) for s in cuts)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        xm = e0 + (lo + hi) / 2 * d
        act = np.abs(xm) > half
        if not act.any():
            return LD(0)
        den = (d[act] ** 2).sum()
        if den > 0:
            s = -(d[act] * (e0[act] - np.sign(xm[act]) * half[act])).sum() / den
            best = min(best, f2(min(max(s, lo), hi)))
    return np.sqrt(best)


def _world_ld(t, f):
    assert t.frame_parent[f] < 0, "world-fixed frames only"
    pl = np.asarray(t.frame_placement, dtype=LD).reshape(-1, 12)[f]
    hl = LD(0) if t.frame_halflen is None else LD(t.frame_halflen[f])
    box = np.asarray(t.frame_box, dtype=LD).reshape(-1, 3)[f] if is_box(t, f) else None
    return pl[:9].reshape(3, 3), pl[9:], LD(t.frame_radius[f]), hl, box


def exact_distance(t, fa, fb):
    """Signed distance of a pair of world-fixed geometry frames from the stored doubles, in longdouble: sphere / capsule pairs by
    the closed forms above, a box against a sphere or capsule by segment_box; a sphere centre inside the box gives minus the depth
    to the nearest face, minus the radius (the definition of the overlap)."""
    Ra, pa, ra, ha, ba = _world_ld(t, fa)
    Rb, pb, rb, hb, bb = _world_ld(t, fb)
    assert ba is None or bb is None, "box / box pairs are not supported"
    if bb is None and ba is not None:
        (Ra, pa, ra, ha, ba), (Rb, pb, rb, hb, bb) = (Rb, pb, rb, hb, bb), (Ra, pa, ra, ha, ba)
    a0, a1 = _ends(Ra, pa, ha)
    if bb is not None:
        l0, l1 = Rb.T @ (a0 - pb), Rb.T @ (a1 - pb)
        d = segment_box(l0, l1, bb)
        if d == 0:
            assert ha == 0, "a capsule axis that meets the box has no reference here"
            return -(bb - np.abs(l0)).min() - ra
        return d - ra
    b0, b1 = _ends(Rb, pb, hb)
    if ha == 0 and hb == 0:
        d = np.sqrt(((pa - pb) ** 2).sum())
    elif ha == 0:
        d = point_segment(pa, b0, b1)
    elif hb == 0:
        d = point_segment(pb, a0, a1)
    else:
        d = segment_segment(a0, a1, b0, b1)
    return d - (ra + rb)


_SCENE = {}


def degenerate_scene():
    """(table, cases): world-fixed geometry on a 2-joint chain; cases = [(frame a, frame b, exact distance, witness_defined)],
    every pair as (a, b) and as (b, a).  Computed once, shared, left unchanged.
    Boxes (one turned, one aligned with the world axes, half extents 0.05 / 0.08 / 0.11) against a capsule (r 0.03, half length
    0.07) or a sphere (r 0.04): generic; axis parallel to a face; axis parallel to an edge, beside the edge; nearest point a vertex;
    an end point nearest to a face; spheres in front of a face, an edge and a vertex; a sphere centre inside the box.
    Capsule pairs: parallel beside each other and staggered; tilted by 1e-3, 1e-6 and 1e-8 rad (both sides of the device's
    denominator test) about the common perpendicular and within the common plane; collinear end to end; crossing axes (distance
    -(ra + rb), normal undefined); a sphere (half length 0) beside and beyond the end of a capsule."""
    if _SCENE:
        return _SCENE["case"]
    t = rt.chain_table(2, seed=1)
    half = (0.05, 0.08, 0.11)
    cases = []

    def put(name, base, Rl, pl, **kw):
        nonlocal t
        Rb, pb = base[:9].reshape(3, 3), base[9:]
        t = t.with_geometry(name, -1, rt.se3(Rb @ Rl, pb + Rb @ np.asarray(pl, dtype=float)), **kw)
        return name

    cap, sph = dict(radius=0.03, halflen=0.07), dict(radius=0.04)
    I3 = np.eye(3)
    for bname, base in (("boxT", rt.se3(rt.rpy(0.4, -0.7, 1.1), [0.5, 0.2, 0.3])), ("boxA", rt.se3(None, [-0.4, 0.6, 0.1]))):
        put(bname, rt.se3(), base[:9].reshape(3, 3), base[9:], box=half)
        others = [
            put(bname + "_generic", base, rt.rpy(0.9, 0.5, -0.3), [0.25, 0.2, -0.18], **cap),
            put(bname + "_face", base, rt.rpy(0.6, 0.0, 0.0), [0.16, 0.01, 0.02], **cap),          # axis in the plane x = 0.16
            put(bname + "_edge", base, I3, [0.10, 0.12, 0.03], **cap),                             # axis along z beside the edge x, y
            put(bname + "_vertex", base, rt.rpy(0.0, 0.9, 0.7), [0.2, 0.22, 0.27], **cap),
            put(bname + "_end", base, rt.rpy(0.0, np.pi / 2, 0.0), [0.2, 0.02, -0.03], **cap),     # axis along x, towards the face
            put(bname + "_sphere_face", base, I3, [0.01, -0.2, 0.03], **sph),
            put(bname + "_sphere_edge", base, I3, [0.12, 0.0, -0.2], **sph),
            put(bname + "_sphere_vertex", base, I3, [-0.1, -0.15, 0.2], **sph),
            put(bname + "_sphere_inside", base, I3, [0.02, -0.05, 0.03], **sph),
        ]
        cases += [(bname, o, o != bname + "_sphere_inside") for o in others]
    baseC = rt.se3(rt.rpy(-0.5, 0.8, 0.2), [0.1, -0.5, 0.4])
    put("capA", baseC, I3, [0.0, 0.0, 0.0], **cap)
    others = [(put("cap_parallel", baseC, I3, [0.1, 0.0, 0.05], **cap), True),
              (put("cap_staggered", baseC, I3, [0.05, 0.0, 0.3], **cap), True),
              (put("cap_collinear", baseC, I3, [0.0, 0.0, 0.3], **cap), True),
              (put("cap_crossing", baseC, rt.rpy(np.pi / 2, 0.0, 0.0), [0.0, 0.01, 0.02], **cap), False),
              (put("sphere_beside", baseC, I3, [0.0, 0.12, 0.03], **sph), True),
              (put("sphere_beyond", baseC, I3, [0.0, 0.0, 0.2], **sph), True)]
    for eps in (1e-3, 1e-6, 1e-8):
        others.append((put(f"cap_tilt_perp_{eps:g}", baseC, rt.rpy(eps, 0.0, 0.0), [0.1, 0.0, 0.02], **cap), True))
        others.append((put(f"cap_tilt_plane_{eps:g}", baseC, rt.rpy(eps, 0.0, 0.0), [0.0, 0.1, 0.02], **cap), True))
    cases += [("capA", o, sep) for o, sep in others]
    out = []
    for a, b, witness in cases:
        for x, y in ((a, b), (b, a)):
            out.append((x, y, float(exact_distance(t, t.frame_id(x), t.frame_id(y))), witness))
    _SCENE["case"] = (t, out)
    return _SCENE["case"]


# ------------------------------------------------------------------------------------------------------------ checker
def checker_distance(t, pair, q):
    """The CPU checker's distance of one pair at q [n][nv]: a problem with this pair as its only constraint row, orc_node_constraints
    at every configuration (how tests/test_many_collision_costs.py reads the distance of a pair row)."""
    from oracle.oracle import Oracle, _p, lib

    q = np.asarray(q, dtype=float)
    nv = t.nv
    running, terminal = workloads.regulation_rows()
    con = workloads.collision_pair_constraints(t, [pair], 0.0)
    oc = Oracle(t, _abi.PackedOcp(nv, [0.01] * 2, list(running), list(terminal), running_constraints=con), 1)
    g, Gx, Gu, nc = np.zeros(8), np.zeros((8, 2 * nv)), np.zeros((8, nv)), C.c_int(0)
    out = np.empty(q.shape[0])
    u = np.zeros(nv)
    for k in range(q.shape[0]):
        x = np.concatenate([q[k], np.zeros(nv)])
        lib().orc_node_constraints(oc._h, 0, _p(x), _p(u), _p(g), _p(Gx), _p(Gu), C.byref(nc))
        assert nc.value == 1
        out[k] = g[0]
    return out


_CHAIN = {}


def chain_case(T=4, seed=71):
    """(table, q [B][T + 1][6], checker dist [B][T + 1][64]) of the 64 pairs of _pairs(64) on the chain: computed once, shared,
    left unchanged."""
    if not _CHAIN:
        t = _chain()
        q = np.random.default_rng(seed).uniform(-1.2, 1.2, (B, T + 1, 6))
        d = np.stack([checker_distance(t, pair, q.reshape(-1, 6)) for pair in _pairs(64)], -1).reshape(B, T + 1, 64)
        _CHAIN["case"] = (t, q, d)
    return _CHAIN["case"]


# --------------------------------------------------------------------------------------------------------------- tests
def test_closed_forms_on_hand_made_cases():
    z = np.zeros(3)
    assert point_segment(np.array([0.0, 3.0, 0.5]), z, np.array([0.0, 0.0, 1.0])) == 3.0
    assert point_segment(np.array([0.0, 3.0, 5.0]), z, np.array([0.0, 0.0, 1.0])) == 5.0
    assert point_segment(np.array([0.0, 3.0, 4.0]), z, z) == 5.0
    e = lambda *v: np.array(v, dtype=float)  # noqa: E731
    assert segment_segment(e(-1, 0, 0), e(1, 0, 0), e(0, -1, 2), e(0, 1, 2)) == 2.0  # crossing: the interior point
    assert segment_segment(e(-1, 0, 0), e(1, 0, 0), e(4, 0, 4), e(4, 0, 8)) == 5.0  # end point against end point
    assert segment_segment(e(-1, 0, 0), e(1, 0, 0), e(-1, 3, 0), e(1, 3, 0)) == 3.0  # parallel
    assert segment_segment(e(-1, 0, 0), e(1, 0, 0), e(0.5, 1, 0), e(0.5, 7, 0)) == 1.0  # end point against the interior


def test_surface_distance_of_sphere_capsule_and_box():
    t = rt.chain_table(2, seed=1)
    t = t.with_geometry("s", -1, rt.se3(None, [1.0, 0.0, 0.0]), 0.25)
    t = t.with_geometry("c", -1, rt.se3(None, [0.0, 2.0, 0.0]), 0.1, 0.5)
    t = t.with_geometry("b", -1, rt.se3(rt.rpy(0.0, 0.0, np.pi / 2), [0.0, 0.0, 3.0]), box=(0.1, 0.2, 0.3))
    q = np.zeros(2)
    f = t.frame_id
    np.testing.assert_allclose(surface_distance(t, f("s"), q, np.array([1.0, 0.25, 0.0])), 0.0, atol=1e-16)
    np.testing.assert_allclose(surface_distance(t, f("s"), q, np.array([1.0, 0.0, 1.0])), 0.75, atol=1e-16)
    np.testing.assert_allclose(surface_distance(t, f("c"), q, np.array([0.1, 2.0, 0.2])), 0.0, atol=1e-16)
    np.testing.assert_allclose(surface_distance(t, f("c"), q, np.array([0.0, 2.0, 0.7])), 0.1, atol=1e-16)  # above the cap
    # the box is turned by 90 degrees about z: its half extents along world x, y, z are 0.2, 0.1, 0.3
    np.testing.assert_allclose(surface_distance(t, f("b"), q, np.array([0.2, 0.05, 3.1])), 0.0, atol=1e-15)
    np.testing.assert_allclose(surface_distance(t, f("b"), q, np.array([0.5, 0.5, 3.0])), 0.5, atol=1e-15)
    np.testing.assert_allclose(surface_distance(t, f("b"), q, np.array([0.0, 0.0, 3.0])), 0.1, atol=1e-15)  # inside: the nearest face


def test_reference_matches_the_checker_on_every_sphere_and_capsule_pair():
    """The 64 pairs of the chain at B x 5 configurations: every pair without a box within 1e-12 of the checker."""
    t, q, d = chain_case()
    pairs = _pairs(64)
    n_checked = 0
    for k, (a, b) in enumerate(pairs):
        if is_box(t, t.frame_id(a)) or is_box(t, t.frame_id(b)):
            continue
        err = np.abs(distance(t, t.frame_id(a), t.frame_id(b), q) - d[..., k]).max()
        assert err <= 1e-12, (a, b, err)
        n_checked += 1
    assert n_checked == 4 + 5 * 8  # self pairs, and the links against four capsules and four spheres
    kinds = {(float(t.frame_halflen[t.frame_id(b)]) > 0.0) for _, b in pairs if not is_box(t, t.frame_id(b))}
    assert kinds == {True, False}


def test_reference_follows_trees_and_prismatic_joints():
    """Sphere / sphere distances against jr.residual (the complex-step reference of tests/test_prismatic.py) on a tree with
    prismatic joints: the same kinematics, the other distance code."""
    name, (t, _, _, (sa, sb)) = next((k, v) for k, v in jr.prismatic_models().items() if k == "tree12p")
    q = np.random.default_rng(3).uniform(-0.5, 0.5, (7, t.nv))
    x = np.concatenate([q, np.zeros_like(q)], -1)
    want = jr.residual(t, _abi.RES_COLLISION, sa, sb, np.zeros(0), x, None)[..., 0]
    np.testing.assert_allclose(distance(t, sa, sb, q), want, rtol=0, atol=1e-15)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the argument checks must come before any call into the library ({name})")


def test_wrapper_refuses_bad_arguments_before_any_gpu_work(monkeypatch):
    from agimus_controller_amd import backend

    t = _chain()
    h = backend.HipOcp.__new__(backend.HipOcp)
    h.table, h.B, h.T, h.nv, h._h, h._m = t, B, 4, 6, None, None
    monkeypatch.setattr(backend, "lib", lambda: _NoLibrary())
    with pytest.raises(ValueError, match="pairs"):
        h.clearance([])
    with pytest.raises(ValueError, match="pairs"):
        h.clearance([("cap1", "cap3", "cap4")])
    with pytest.raises(ValueError, match="pairs"):
        h.clearance([3])
    with pytest.raises(ValueError, match="pairs.*no frame 'nothing'"):
        h.clearance([("cap1", "nothing")])
    for bad in (np.zeros((B, 5, 7)), np.zeros((B + 1, 5, 6)), np.zeros((B, 0, 6)), np.zeros((B * 5, 6))):
        with pytest.raises(ValueError, match="q: expected shape"):
            h.clearance([("cap1", "cap3")], q=bad)


def test_segment_box_on_hand_made_cases():
    h = (1.0, 2.0, 3.0)
    assert segment_box((4, 0, 0), (4, 0, 0), h) == 3.0                        # a point in front of a face
    assert segment_box((4, 6, 0), (4, 6, 0), h) == 5.0                        # ... of an edge
    assert segment_box((3, 4, 4), (3, 4, 4), h) == 3.0                        # ... of a vertex (2, 2, 1)
    assert segment_box((5, -9, 1), (5, 9, 1), h) == 4.0                       # parallel to a face
    assert segment_box((4, 6, -9), (4, 6, 9), h) == 5.0                       # parallel to an edge
    assert segment_box((9, 0, 0), (3, 0, 0), h) == 2.0                        # an end point
    assert segment_box((4, 0, 0), (0, 4, 0), h) == np.sqrt(LD(0.5))           # passes the edge (1, 2, .) at 45 degrees: |(1, 2) - (1.5, 2.5)|
    assert segment_box((-9, 0, 0), (9, 0, 0), h) == 0.0                       # through the box
    assert segment_box((0.5, 0, 0), (0.5, 0, 0), h) == 0.0


def test_checker_matches_the_exact_reference_on_box_and_degenerate_capsule_pairs():
    """Every pair of degenerate_scene, both orders, within 1e-12 of the longdouble reference (the bound of the device test)."""
    t, cases = degenerate_scene()
    assert len(cases) == 2 * (2 * 9 + 12)
    q = np.zeros((1, t.nv))
    worst = 0.0
    bad = []
    for a, b, want, _ in cases:
        got = checker_distance(t, (a, b), q)[0]
        worst = max(worst, abs(got - want))
        print(f"{a} / {b}: checker {got:.17g} exact {want:.17g} diff {got - want:.2e}")
        if not abs(got - want) <= 1e-12:
            bad.append((a, b, got, want))
    assert not bad, bad
    inside = [w for a, b, w, _ in cases if "inside" in a + b]
    crossing = [w for a, b, w, _ in cases if "crossing" in a + b]
    assert all(w < -0.04 for w in inside) and all(abs(w + 0.06) < 1e-15 for w in crossing)
    assert sum(w > 0 for _, _, w, _ in cases) == len(cases) - len(inside) - len(crossing)

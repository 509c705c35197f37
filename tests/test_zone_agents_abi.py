"""Agents in polygon zones (include/crowdstep_state.h, cs_zone_agents) without a GPU: the header declares the entry points
and the binding table binds them with these signatures, the cross-compiled library exports them, the ctypes Zone and
ZoneAgent and the numpy dtypes have the layout of the C structs, the C++ mirror compiles, and the restatement of the rule
(tests/zones_reference.py), which the GPU tests compare the engine with, holds on hand cases: what follows from the rule
(the rectangle is CS_SEL_RECT, tilings cover every point an odd number of times, exactly once where the arithmetic is
exact) is checked here on the restatement alone."""
import ctypes
import os
import re
import subprocess

import numpy as np

from rmf_crowdsim_amd import _abi, _native
from rmf_crowdsim_amd.simulation import AGENT_DTYPE, ZONE_AGENT_DTYPE, ZONE_DTYPE
from zones_reference import box, crossings, in_rect, in_ring, rect_ring, zone_agents, zones_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("cs_zone_agents", "cs_mesh_zone_agents")
GRID = dict(width=40.0, height=40.0, cell_size=2.0, offset=(-20.0, -20.0))  # x and y in [-20, 20)
INF = float("inf")


def _header():
    return open(os.path.join(ROOT, "include", "crowdstep_state.h")).read()


def test_the_state_header_declares_and_binds_the_zone_calls():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(cs_[a-z_0-9]+)\s*\(", text)))
    C = ctypes
    want = (C.c_size_t, [C.c_void_p, C.POINTER(_abi.Zone), C.c_size_t, C.POINTER(C.c_double), C.c_size_t,
                         C.POINTER(_abi.Selection), C.POINTER(C.c_uint64), C.POINTER(_abi.ZoneAgent), C.c_size_t])
    for name in CALLS:
        assert name in declared and _abi.STATE_SYMBOLS[name] == want, name
    assert sorted(_abi.STATE_SYMBOLS) == declared
    for call in CALLS:  # the argument list of the header, type by type
        args = re.search(r"\bsize_t " + call + r"\((.*?)\);", text, flags=re.S).group(1)
        kinds = [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]
        assert [re.sub(r" [a-z_0-9]+$", "", k) for k in kinds] == [
            "cs_mesh*" if "mesh" in call else "cs_engine*", "const cs_zone*", "size_t", "const double*", "size_t",
            "const cs_selection*", "uint64_t*", "cs_zone_agent*", "size_t"], kinds
        assert [k.split(" ")[-1] for k in kinds[1:]] == ["zones", "n", "vertices_xy", "n_vertices", "filter", "out_counts",
                                                         "out", "cap"]
    assert "Agents in polygon zones" in _header()
    assert int(re.search(r"#define\s+CS_ZONES_MAX\s+(\d+)u", text).group(1)) == _abi.CS_ZONES_MAX == 65536
    assert re.search(r"#define\s+CS_ZONE_VERTICES_MAX\s+\(1u << 20\)", text) and _abi.CS_ZONE_VERTICES_MAX == 1 << 20


def test_hip_library_exports_the_zone_calls():
    lib = _abi.bind_state(ctypes.CDLL(_native.build()))
    for name in CALLS:
        fn = getattr(lib, name)  # (AttributeError: the symbol is missing)
        restype, argtypes = _abi.STATE_SYMBOLS[name]
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_the_ctypes_structs_and_the_dtypes_have_the_layout_of_the_c_structs(tmp_path):
    zone = [f for f, _ in _abi.Zone._fields_]
    row = [f for f, _ in _abi.ZoneAgent._fields_]
    assert zone == ["first", "count", "flags"] == list(ZONE_DTYPE.names)
    assert row == ["zone", "id"] == list(ZONE_AGENT_DTYPE.names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "crowdstep_state.h"\nint main(void) {\n'
                   '  printf("%zu\\n%zu\\n", sizeof(cs_zone), sizeof(cs_zone_agent));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(cs_zone, {f}));\n' for f in zone)
                   + "".join(f'  printf("%zu\\n", offsetof(cs_zone_agent, {f}));\n' for f in row)
                   + '  printf("%zu\\n", sizeof(cs_selection));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got[0] == ctypes.sizeof(_abi.Zone) == ZONE_DTYPE.itemsize == 16
    assert got[1] == ctypes.sizeof(_abi.ZoneAgent) == ZONE_AGENT_DTYPE.itemsize == 16
    assert got[2:5] == [getattr(_abi.Zone, f).offset for f in zone] == [ZONE_DTYPE.fields[f][1] for f in zone] == [0, 8, 12]
    assert got[5:7] == [getattr(_abi.ZoneAgent, f).offset for f in row] == [ZONE_AGENT_DTYPE.fields[f][1] for f in row] == [0, 8]
    assert [ZONE_DTYPE.fields[f][0] for f in zone] == [np.dtype("u8"), np.dtype("u4"), np.dtype("u4")]
    assert [ZONE_AGENT_DTYPE.fields[f][0] for f in row] == [np.dtype("u8")] * 2
    assert got[7] == ctypes.sizeof(_abi.Selection) == 104


def test_cpp_mirror_with_the_zone_calls_compiles():
    from test_gpu_cpp_api import build_cpp_test
    assert os.path.exists(build_cpp_test("test_zone_agents"))


def test_zones_array_lays_the_rings_out_one_after_the_other():
    zones, vertices = zones_array([rect_ring(0, 0, 1, 1), [(0, 0), (2, 0), (1, 3)], rect_ring(5, 5, 6, 7)])
    assert zones.dtype == ZONE_DTYPE and zones["first"].tolist() == [0, 4, 7] and zones["count"].tolist() == [4, 3, 4]
    assert not zones["flags"].any() and vertices.shape == (11, 2) and vertices[4:7].tolist() == [[0, 0], [2, 0], [1, 3]]
    again = zones_array((zones, vertices))
    assert again[0].tobytes() == zones.tobytes() and again[1].tobytes() == vertices.tobytes()
    zones, vertices = zones_array([])
    assert zones.shape == (0,) and vertices.shape == (0, 2)


def _edge_points(x0, y0, x1, y1):
    """points on every edge and corner of the rectangle, one ulp either side of each, inside and outside"""
    xs = [x0, x1, (x0 + x1) / 2, x0 - 1.0, x1 + 1.0]
    ys = [y0, y1, (y0 + y1) / 2, y0 - 1.0, y1 + 1.0]
    xs += [np.nextafter(v, s) for v in (x0, x1) for s in (-INF, INF)]
    ys += [np.nextafter(v, s) for v in (y0, y1) for s in (-INF, INF)]
    gx, gy = np.meshgrid(np.array(xs, dtype=np.float64), np.array(ys, dtype=np.float64))
    return gx.ravel(), gy.ravel()


def test_the_rectangle_is_the_rect_term_in_either_winding():
    for x0, y0, x1, y1 in ((0.0, 0.0, 4.0, 2.0), (-3.7, 1.1, 0.3, 1.9), (0.1, 0.2, 0.7, 12.3), (1e6 + 0.1, -5.0, 1e6 + 0.3, 7.7)):
        x, y = _edge_points(x0, y0, x1, y1)
        want = in_rect(x, y, x0, y0, x1, y1)
        assert 0 < want.sum() < len(want)
        for reverse in (False, True):
            for shift in range(4):  # every vertex as the first
                ring = np.roll(rect_ring(x0, y0, x1, y1, reverse), shift, axis=0)
                assert (in_ring(x, y, ring) == want).all(), (x0, y0, x1, y1, reverse, shift)


def test_hand_cases_of_the_ring_test():
    # a concave ring: an L (the notch 2 <= x, 2 <= y is outside)
    L = np.array([(0, 0), (4, 0), (4, 2), (2, 2), (2, 4), (0, 4)], dtype=np.float64)
    pts = {(1, 1): True, (3, 1): True, (1, 3): True, (3, 3): False, (2, 2): False, (2, 3): False, (3, 2): False,
           (1.999, 3): True, (0, 0): True, (4, 0): False, (0, 4): False, (0, 2): True, (4, 1): False, (2, 0): True}
    for (x, y), want in pts.items():
        assert bool(in_ring([x], [y], L)[0]) is want, (x, y)
        assert bool(in_ring([x], [y], L[::-1])[0]) is want, (x, y, "reversed")
    # a bow tie (self-intersecting): two triangles that meet at (2, 2); even-odd.  The meeting point lies ON both
    # diagonals (c == 0 exactly: no crossing) and left of the edge x == 4 (one crossing): it is in, by the rule
    bow = np.array([(0, 0), (4, 4), (4, 0), (0, 4)], dtype=np.float64)
    assert crossings([2.0], [2.0], bow)[0] == 1
    for (x, y), want in {(3.5, 2): True, (0.5, 2): True, (2, 0.5): False, (2, 3.5): False, (2, 2): True, (5, 2): False}.items():
        assert bool(in_ring([x], [y], bow)[0]) is want, (x, y)
    # a horizontal edge through the point: it never straddles, the verticals decide as for a rectangle
    sq = rect_ring(0, 0, 2, 2)
    assert crossings([1.0], [0.0], sq)[0] == 1 and in_ring([1.0], [0.0], sq)[0]        # on the low edge: in
    assert crossings([1.0], [2.0], sq)[0] == 0 and not in_ring([1.0], [2.0], sq)[0]    # on the high edge: out
    assert crossings([-1.0], [0.0], sq)[0] == 2 and not in_ring([-1.0], [0.0], sq)[0]  # left of it: two crossings, and the box
    # a point on a vertex: c == 0 exactly for both edges that end there, so only another edge can put it in.  Of the
    # square's vertices the low corner is in (the edge x == 2 crosses), as for CS_SEL_RECT; a triangle's are all out
    tri = np.array([(0, 0), (4, 1), (1, 3)], dtype=np.float64)
    assert [bool(in_ring([x], [y], tri)[0]) for x, y in tri] == [False, False, False]
    assert [bool(in_ring([x], [y], sq)[0]) for x, y in sq] == [True, False, False, False]
    # a zero-area ring: nobody, on it or off it
    flat = np.array([(0, 0), (2, 2), (4, 4), (2, 2)], dtype=np.float64)
    line = np.array([(0, 1), (3, 1), (5, 1)], dtype=np.float64)
    x, y = np.array([1.0, 2.0, 3.0, 0.0, 1.0]), np.array([1.0, 2.0, 3.0, 0.0, 2.0])
    assert not in_ring(x, y, flat).any() and not in_ring(x, y, line).any()
    assert box(flat) == (0.0, 4.0, 0.0, 4.0) and box(line) == (0.0, 5.0, 1.0, 1.0)
    # the box is part of the rule: nothing outside it, whatever the crossings say
    far = np.array([-1e300, 1e300, 0.0]), np.array([1.0, 1.0, 1e300])
    assert not in_ring(*far, tri).any()


def _tiling(xs, ys, rng):
    """the cells of the lattice xs x ys, each cut into two triangles along a diagonal chosen at random, with windings and
    first vertices chosen at random: rings that tile [xs[0], xs[-1]] x [ys[0], ys[-1]] with matching vertices"""
    rings = []
    for i in range(len(xs) - 1):
        for j in range(len(ys) - 1):
            a, b, c, d = (xs[i], ys[j]), (xs[i + 1], ys[j]), (xs[i + 1], ys[j + 1]), (xs[i], ys[j + 1])
            pair = [(a, b, c), (a, c, d)] if rng.integers(2) else [(a, b, d), (b, c, d)]
            for t in pair:
                t = np.roll(np.array(t, dtype=np.float64), int(rng.integers(3)), axis=0)
                rings.append(t[::-1].copy() if rng.integers(2) else t)
    return rings


def test_a_dyadic_tiling_holds_every_point_exactly_once():
    """4 x 4 cells of 1/4 cut into triangles; points on a lattice of 1/16: on edges, on vertices, inside.  All the
    arithmetic is exact, so every point of [0, 1) x [0, 1) is in exactly one triangle (the high edges x == 1 and y == 1
    belong to nobody, as those of a rectangle)."""
    rng = np.random.default_rng(5)
    xs = ys = np.arange(5) / 4.0
    gx, gy = np.meshgrid(np.arange(17) / 16.0, np.arange(17) / 16.0)
    x, y = gx.ravel(), gy.ravel()
    for _ in range(4):
        rings = _tiling(xs, ys, rng)
        assert len(rings) == 32
        times = sum(in_ring(x, y, r).astype(np.int64) for r in rings)
        inside = (x < 1.0) & (y < 1.0)
        assert (times[inside] == 1).all() and (times[~inside] == 0).all()


def test_random_tilings_hold_every_point_an_odd_number_of_times():
    """Lattices with non-dyadic coordinates, warped so that no edge but the outer ones is axis-aligned; random points and
    points ON the shared edges as well as rounding allows.  Shared edges are judged alike from either side, so every
    point strictly inside the region is in an odd number of triangles."""
    rng = np.random.default_rng(6)
    odd_total = more = 0
    for _ in range(6):
        n = 5
        xs, ys = np.sort(rng.uniform(0.1, 9.9, n - 1)), np.sort(rng.uniform(0.1, 9.9, n - 1))
        xs, ys = np.concatenate([[0.0], xs, [10.0]]), np.concatenate([[0.0], ys, [10.0]])
        # warp the inner lattice points: each moves a little, consistently for every triangle that uses it
        px, py = np.meshgrid(xs, ys, indexing="ij")
        px, py = px.copy(), py.copy()
        px[1:-1, 1:-1] += rng.uniform(-0.03, 0.03, (n - 1, n - 1))
        py[1:-1, 1:-1] += rng.uniform(-0.03, 0.03, (n - 1, n - 1))
        rings = []
        for i in range(n):
            for j in range(n):
                a, b, c, d = [(px[u, v], py[u, v]) for u, v in ((i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1))]
                for t in ([(a, b, c), (a, c, d)] if rng.integers(2) else [(a, b, d), (b, c, d)]):
                    t = np.roll(np.array(t, dtype=np.float64), int(rng.integers(3)), axis=0)
                    rings.append(t[::-1].copy() if rng.integers(2) else t)
        x, y = rng.uniform(0.2, 9.8, 3000), rng.uniform(0.2, 9.8, 3000)
        on = []  # points on the shared edges, as well as f64 can place them
        for r in rings:
            s = rng.uniform(0.0, 1.0, 4)
            on.append(np.column_stack([r[0, 0] + s * (r[1, 0] - r[0, 0]), r[0, 1] + s * (r[1, 1] - r[0, 1])]))
        on = np.concatenate(on)
        on = on[(on[:, 0] > 0.2) & (on[:, 0] < 9.8) & (on[:, 1] > 0.2) & (on[:, 1] < 9.8)]
        x, y = np.concatenate([x, on[:, 0]]), np.concatenate([y, on[:, 1]])
        times = sum(in_ring(x, y, r).astype(np.int64) for r in rings)
        assert (times % 2 == 1).all(), (times[times % 2 == 0][:5], x[times % 2 == 0][:5], y[times % 2 == 0][:5])
        odd_total += len(times)
        more += int((times > 1).sum())
    print(f"{odd_total} points, each in an odd number of triangles; {more} of them in more than one")


def _records(points, first_id=10):
    out = np.zeros(len(points), dtype=AGENT_DTYPE)
    for k, (x, y) in enumerate(points):
        out[k] = (first_id + k, x, y, 0.0, 0.0, 0, 2.0)
    return out


def test_the_restatement_lists_participants_by_zone_and_id():
    rec = _records([(1.0, 1.0), (3.0, 1.0), (-25.0, 1.0), (1.0, 25.0), (float("nan"), 1.0), (19.999, 19.999), (20.0, 0.0)])
    rec["id"] = [16, 11, 12, 13, 14, 15, 10]
    zones, vertices = zones_array([rect_ring(0, 0, 2, 2), rect_ring(-30, -30, 30, 30), [(2.5, 0), (3.5, 0), (3, 5)],
                                   rect_ring(100, 100, 101, 101)])
    rows, counts = zone_agents(rec, GRID, zones, vertices)
    assert rows["zone"].tolist() == [0, 1, 1, 1, 2] and rows["id"].tolist() == [16, 11, 15, 16, 11]  # (outsiders and NaN: never)
    assert counts.tolist() == [1, 3, 1, 0] and counts.dtype == np.uint64 and rows.dtype == ZONE_AGENT_DTYPE
    rows, counts = zone_agents(rec, GRID, zones, vertices, mask=rec["id"] != 11)
    assert rows["id"].tolist() == [16, 15, 16] and counts.tolist() == [1, 2, 0, 0]
    shared = (np.array([(0, 4, 0), (2, 4, 0)], dtype=ZONE_DTYPE), np.array([(0, 0), (2, 0), (2, 2), (0, 2), (0, 0), (2, 0)], dtype=np.float64))
    rows, counts = zone_agents(rec, GRID, *shared)  # runs that overlap: the second ring is (2,2) (0,2) (0,0) (2,0)
    assert counts.tolist() == [1, 1]

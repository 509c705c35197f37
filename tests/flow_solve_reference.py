"""The rule of cs_flow_field_solve (include/crowdstep_state.h, "Solving a flow field on the device") restated for the tests:
plain sweeps to the fixed point in numpy f64, every operation the one the header spells, rounded once.  It shares nothing
with the package's heap Dijkstra (flow_field_solve_host) and nothing with the device's tiles; IEEE addition is monotone, so
all three reach the same bits.  Slow: for rasters of a few thousand bins.  Also the scenes the GPU tests share."""
import numpy as np

STEPS = tuple((dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy)
F64 = np.float64


def lengths(cell):
    cw, ch = F64(cell[0]), F64(cell[1])
    diag = np.sqrt(cw * cw + ch * ch)
    return [diag if dx and dy else cw if dx else ch for dx, dy in STEPS]


def slowness_of(shape, slowness, counts, density_weight):
    s = np.ones(shape, dtype=F64) if slowness is None else np.asarray(slowness, dtype=np.float32).astype(F64)
    if F64(density_weight) != 0.0:
        s = s * (F64(1.0) + F64(density_weight) * np.asarray(counts, dtype=np.uint32).astype(F64))
    return s


def allowed_steps(blocked):
    """per step of STEPS a bool (ny, nx): the walker may take it from that bin"""
    ny, nx = blocked.shape
    wall = np.pad(blocked, 1, constant_values=True)  # (outside the raster: no step leads there)
    at = lambda dx, dy: wall[1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]  # noqa: E731
    out = []
    for dx, dy in STEPS:
        ok = ~blocked & ~at(dx, dy)
        if dx and dy:
            ok = ok & ~at(dx, 0) & ~at(0, dy)
        out.append(ok)
    return out


def solve(blocked, goals, cell, speed, slowness=None, counts=None, density_weight=0.0):
    """-> (vectors float32 (ny, nx, 2), dist float64 (ny, nx), reached, sweeps)"""
    goals = np.asarray(goals) != 0
    blocked = np.zeros(goals.shape, dtype=bool) if blocked is None else np.asarray(blocked) != 0
    ny, nx = goals.shape
    lens = lengths(cell)
    s = slowness_of(goals.shape, slowness, counts, density_weight)
    ok = allowed_steps(blocked)
    with np.errstate(all="ignore"):
        cost = [lens[k] * s for k in range(8)]
        dist = np.where(goals & ~blocked, F64(0.0), F64(np.inf))

        def towards(k, d):
            dx, dy = STEPS[k]
            far = np.pad(d, 1, constant_values=np.inf)
            return np.where(ok[k], far[1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx] + cost[k], F64(np.inf))

        sweeps = 0
        while True:
            new = dist
            for k in range(8):
                new = np.minimum(new, towards(k, dist))
            sweeps += 1
            if new.tobytes() == dist.tobytes():
                break
            assert sweeps <= nx * ny + 1
            dist = new
        best = np.full((ny, nx), np.inf)
        pick = np.full((ny, nx), -1, dtype=np.int64)
        for k in range(8):
            c = towards(k, dist)
            better = c < best
            best = np.where(better, c, best)
            pick = np.where(better, k, pick)
        table = np.zeros((8, 2), dtype=np.float32)
        for k, (dx, dy) in enumerate(STEPS):
            sx, sy = F64(dx) * F64(cell[0]), F64(dy) * F64(cell[1])
            table[k] = (np.float32((F64(speed) * sx) / lens[k]), np.float32((F64(speed) * sy) / lens[k]))
    finite = np.isfinite(dist)
    vectors = np.full((ny, nx, 2), np.nan, dtype=np.float32)
    moving = finite & ~goals & (pick >= 0)
    vectors[moving] = table[pick[moving]]
    vectors[finite & goals] = 0.0
    return vectors, dist, int(finite.sum()), sweeps


# ---- scenes -----------------------------------------------------------------------------------------------------------

def random_walls(ny, nx, seed, share, goal_bins):
    """`share` of the bins blocked at random, the goals free"""
    rng = np.random.default_rng(seed)
    blocked = rng.random((ny, nx)) < share
    goals = np.zeros((ny, nx), dtype=bool)
    for ix, iy in goal_bins:
        goals[iy, ix] = True
        blocked[iy, ix] = False
    return blocked, goals


def issue_case():
    """70 x 45, default_rng(1), 30 % blocked, goals at (5, 3) and (60, 40)"""
    return random_walls(45, 70, 1, 0.3, [(5, 3), (60, 40)])


def serpentine(ny=40, nx=96, every=4):
    """full-height walls every `every` columns with one-bin gaps alternating top and bottom, the goal in one corner"""
    blocked = np.zeros((ny, nx), dtype=bool)
    for n, ix in enumerate(range(every - 1, nx - 1, every)):
        blocked[:, ix] = True
        blocked[0 if n % 2 else ny - 1, ix] = False
    goals = np.zeros((ny, nx), dtype=bool)
    goals[0, 0] = True
    return blocked, goals


def spiral(n=67):
    """a square spiral corridor one bin wide between walls one bin thick, the goal at its middle"""
    blocked = np.ones((n, n), dtype=bool)
    x = y = 0
    dx, dy = 1, 0
    blocked[0, 0] = False
    while True:
        moved = 0
        while True:
            jx, jy = x + dx, y + dy
            kx, ky = jx + dx, jy + dy  # (the bin after the next must not be corridor already: a wall stays between)
            if not (0 <= jx < n and 0 <= jy < n) or not blocked[jy, jx]:
                break
            if 0 <= kx < n and 0 <= ky < n and not blocked[ky, kx]:
                break
            x, y = jx, jy
            blocked[y, x] = False
            moved += 1
        if moved < 2:
            break
        dx, dy = -dy, dx
    goals = np.zeros((n, n), dtype=bool)
    goals[y, x] = True
    return blocked, goals


__all__ = ["STEPS", "solve", "lengths", "random_walls", "issue_case", "serpentine", "spiral"]

"""The clusters of agents under a distance on a tile mesh (cs_mesh_agent_clusters; NativeTileMesh.agent_clusters /
count_clusters), in process and over two ranks: every tile clusters its own agents, the members near a cut travel as band
records with their local label, the labels linked across cuts are merged, and the mesh gives the single engine's answer:
ids, labels, sizes and boxes byte for byte, the sums under their bound (tests/clusters_reference.py).  No halo exchange is
made for it: the next steps of the mesh are those of a mesh that never asked."""
import numpy as np
import pytest

from rmf_crowdsim_amd import LocationHash2D, NoLocalPlan, Simulation, StubHighLevelPlan, _abi
from rmf_crowdsim_amd.tiles import NativeTileMesh
from close_pairs_reference import last_error, roles
from clusters_reference import agent_clusters, agree, clusters, same_table
from select_reference import selection
from test_gpu_close_pairs_mesh import _pair

pytestmark = pytest.mark.gpu
INF = float("inf")
GRID = dict(width=60.0, height=60.0, cell_size=2.0, offset=(0.0, 0.0))  # 30 x 30 cells; 2 x 1 tiles cut at x = 30 m


def _same(mesh, single, rec, grid, distance, sel=None, min_size=1, cols=(None, None, None), name="", cache=None):
    """mesh == single engine == restatement; ids, labels, sizes and boxes of mesh and engine byte for byte"""
    want = agree(single, rec, grid, distance, sel, min_size, cols, name + " (engine)", cache)
    agree(mesh, rec, grid, distance, sel, min_size, cols, name + " (mesh)", cache)
    caps = (len(want[0]) + 1, len(want[2]) + 1)
    e = agent_clusters(single, distance, sel, min_size, *caps, fill=0xCD)
    m = agent_clusters(mesh, distance, sel, min_size, *caps, fill=0xCD)
    assert e[:3] == m[:3] == (0, len(want[0]), len(want[2])), name
    assert e[3].tobytes() == m[3].tobytes() and e[4].tobytes() == m[4].tobytes(), name
    for f in ("label", "size", "min_x", "min_y", "max_x", "max_y"):
        assert e[5][f].tobytes() == m[5][f].tobytes(), (name, f)
    return want


@pytest.mark.parametrize("shape", [(2, 1), (1, 2), (2, 2)])
def test_a_mesh_clusters_like_one_engine(shape):
    mesh, single, led, grid = _pair(shape, 1)
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes()
    assert int((mesh.tile_counts() > 0).sum()) >= 2
    cols = led.columns(rec)
    cell = grid["cell_size"]
    speed = np.hypot(rec["vx"].astype(np.float64), rec["vy"].astype(np.float64))
    slow = selection(_abi.CS_SEL_SPEED, speed_lo=0.0, speed_hi=float(np.median(speed)))
    cache = {}
    for distance in (0.0, 0.3 * cell, 0.7 * cell, cell):  # (cell: the most a mesh with one halo cell allows)
        want = _same(mesh, single, rec, grid, distance, None, 1, cols, f"{shape}, distance {distance}", cache)
        if distance >= 0.7 * cell:
            # clusters across the cuts are among them: a box that holds a cut strictly inside, by the restatement alone
            t = want[2]
            cuts_x = [120.0] if shape[0] == 2 else []
            cuts_y = [120.0] if shape[1] == 2 else []
            across = sum(int(((t["min_x"] < c) & (t["max_x"] >= c)).sum()) for c in cuts_x) + \
                sum(int(((t["min_y"] < c) & (t["max_y"] >= c)).sum()) for c in cuts_y)
            print(f"{shape}, distance {distance}: {len(t)} clusters, {across} of them across a cut")
            assert across > 0
    _same(mesh, single, rec, grid, cell, slow, 1, cols, f"{shape}, the slow half", cache)
    _same(mesh, single, rec, grid, cell, None, 3, cols, f"{shape}, min_size 3", cache)
    # the Python surface of the mesh
    want = clusters(rec, grid, cell, None, 2, cache)
    ids, labels, table = mesh.agent_clusters(cell, min_size=2)
    assert ids.tolist() == want[0].tolist() and labels.tolist() == want[1].tolist()
    assert table["label"].tolist() == want[2]["label"].tolist() and table["size"].tolist() == want[2]["size"].tolist()
    assert mesh.count_clusters(cell, min_size=2) == (len(want[2]), len(want[0]))
    assert mesh.agent_clusters(cell, limit=3)[0].tolist() == clusters(rec, grid, cell, cache=cache)[0][:3].tolist()
    assert mesh.read_agents().tobytes() == rec.tobytes()
    for t in (mesh, single):
        for _ in range(3):
            t.step(0.05)
    assert mesh.read_agents().tobytes() == single.read_agents().tobytes()


def _zigzag(n=41):
    """n points that alternate between the two sides of the cut at x = 30: neighbours in the chain are 0.53 m apart and
    stand on different tiles, agents of one side are 0.7 m apart"""
    k = np.arange(n)
    return np.stack([np.where(k % 2 == 0, 29.8, 30.2), 20.0 + 0.35 * k], axis=1)


def test_a_chain_that_zigzags_across_a_cut_and_the_distance_limit():
    pts = _zigzag()
    rng = np.random.default_rng(37)
    order = rng.permutation(len(pts))
    order[np.nonzero(order == 20)[0][0]], order[0] = order[0], 20  # (the smallest id mid-chain)
    extra = np.array([[10.0, 10.0], [10.4, 10.0], [50.0, 50.0]])  # a pair and a loner far from the cut
    mesh = NativeTileMesh(LocationHash2D(**GRID), (2, 1), 1)
    lone = NativeTileMesh(LocationHash2D(**GRID), (1, 1), 1)
    single = Simulation(LocationHash2D(**GRID))
    ids = None
    for t in (mesh, lone, single):
        ids = t.add_agents(np.concatenate([pts[order], extra]), StubHighLevelPlan((0.0, 0.0)), NoLocalPlan(), 2.0)
    rec = single.read_agents()
    assert rec.tobytes() == mesh.read_agents().tobytes() == lone.read_agents().tobytes()
    assert (mesh.tile_counts() >= 20).all()
    # every tile alone sees no link in the chain: by the restatement on either side of the cut
    for side in (rec["x"] < 30.0, rec["x"] >= 30.0):
        assert int(clusters(rec, GRID, 0.6, side)[2]["size"].max()) <= 2  # (the pair far from the cut, nothing larger)
    want = _same(mesh, single, rec, GRID, 0.6, name="the zigzag")
    assert want[2]["size"].tolist() == [41, 2, 1] and int(want[2]["label"][0]) == min(int(i) for i in ids)
    _same(lone, single, rec, GRID, 0.6, name="the zigzag on one tile")
    _same(mesh, single, rec, GRID, 0.6, None, 3, name="the zigzag, min_size 3")
    _same(mesh, single, rec, GRID, 0.5, name="below the spacing")
    # a distance above halo_cells * cell_size is refused on more than one tile, and the mesh stays usable
    limit = GRID["cell_size"]
    above = float(np.nextafter(limit, INF))
    for caps in ((None, None), (8, 8)):
        rc, na, nc, g_ids, g_lab, g_tab = agent_clusters(mesh, above, None, 1, *caps, fill=0xAB)
        assert rc == 3 and "halo_cells" in last_error(mesh) and na == nc == 2 ** 62
        if caps[0]:
            assert all((arr.view(np.uint8) == 0xAB).all() for arr in (g_ids, g_lab, g_tab))
    assert agent_clusters(mesh, INF)[0] == 3
    _same(mesh, single, rec, GRID, limit, name="at the limit")
    _same(lone, single, rec, GRID, above, name="one tile has no limit")
    _same(lone, single, rec, GRID, INF, name="one tile, +inf")
    for t in (mesh, single):
        t.step(0.05)
    assert mesh.read_agents().tobytes() == single.read_agents().tobytes()


def _two_rank_cases():
    """(distance, members, min_size): the cut of the 2 x 1 mesh of the two ranks lies at x = 30 m; the limit is 2 m"""
    box = selection(_abi.CS_SEL_RECT, x0=24.0, y0=22.5, x1=37.25, y1=36.0)  # across the cut
    return [(0.0, None, 1), (1.2, None, 1), (2.0, None, 2), (1.5, box, 1)]


def _two_rank_answers(t):
    out = []
    for distance, sel, min_size in _two_rank_cases():
        rc, na, nc, _, _, _ = agent_clusters(t, distance, sel, min_size)
        got = agent_clusters(t, distance, sel, min_size, na + 2, nc + 2, fill=0xEE)
        few = agent_clusters(t, distance, sel, min_size, 5, 3, fill=0xEE)
        out.append((rc, na, nc, got[:3], got[3].tobytes(), got[4].tobytes(), got[5], few[3].tobytes(), few[5]["label"].tobytes()))
    return out


def _rank_clusters(rank, world, port, out_path):
    import os
    import pickle
    import torch.distributed as dist
    from rmf_crowdsim_amd.tiles import TorchHostTransport
    from test_gpu_agent_write_mesh import GRID, _scene
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mesh = NativeTileMesh(LocationHash2D(**GRID), (2, 1), 1, device=0, rank=rank, n_ranks=world,
                              host_transport=TorchHostTransport(dist))
        _scene(mesh)
        for _ in range(25):
            mesh.step(0.05, report=False)
        notes = {"before": mesh.read_agents(), "answers": _two_rank_answers(mesh)}
        notes["refused"] = agent_clusters(mesh, 2.5)[0] == 3 and agent_clusters(mesh, float("nan"), None, 1, 4, 4)[0] == 3
        notes["python"] = mesh.agent_clusters(2.0, min_size=2)
        for _ in range(5):
            mesh.agent_clusters(2.0, limit=8)
            mesh.step(0.05, report=False)
        notes["agents"] = mesh.read_agents()
        with open(f"{out_path}.{rank}", "wb") as f:
            pickle.dump(notes, f)
    finally:
        dist.destroy_process_group()


def test_two_ranks_over_a_host_transport_cluster_like_one_engine(tmp_path):
    """Two ranks (2 x 1 tiles) over torch.distributed / gloo sharing the GPU: the band records, the label links and the
    answer travel through the host transport's gathers, every rank gets the whole answer, the single engine's, and steps
    on as it."""
    import pickle
    import torch.multiprocessing as mp
    from test_gpu_agent_write_mesh import GRID, _scene
    ctx = mp.get_context("spawn")
    out = str(tmp_path / "clusters.pkl")
    procs = [ctx.Process(target=_rank_clusters, args=(r, 2, 29811, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0
    notes = []
    for r in range(2):
        with open(f"{out}.{r}", "rb") as f:
            notes.append(pickle.load(f))
    single = Simulation(LocationHash2D(**GRID))
    _scene(single)
    for _ in range(25):
        single.step(0.05, report=False)
    before = single.read_agents()
    want = _two_rank_answers(single)
    t = clusters(before, GRID, 2.0, None, 2)[2]
    assert int(((t["min_x"] < 30.0) & (t["max_x"] >= 30.0)).sum()) > 0  # (a cluster of agents of both ranks)
    assert all(w[0] == 0 for w in want) and want[1][2] > 1 and want[2][2] == len(t)
    listed = single.agent_clusters(2.0, min_size=2)
    for _ in range(5):
        single.step(0.05, report=False)
    end = single.read_agents()
    for n in notes:
        assert n["before"].tobytes() == before.tobytes()
        assert n["refused"]
        for got, w, (distance, sel, min_size) in zip(n["answers"], want, _two_rank_cases()):
            assert got[:6] == w[:6] and got[7:] == w[7:]  # rc, counts, ids and labels: the single engine's bytes
            mask = None if sel is None else roles(sel, None, before)[0]
            _, _, table, absum = clusters(before, GRID, distance, mask, min_size)
            same_table(got[6][:got[2]], table, absum, f"two ranks, distance {distance}")  # (the sums under their bound)
            assert (got[6][got[2]:].view(np.uint8) == 0xEE).all()
        assert n["python"][0].tobytes() == listed[0].tobytes() and n["python"][1].tobytes() == listed[1].tobytes()
        assert n["python"][2]["size"].tobytes() == listed[2]["size"].tobytes()
        assert len(end) > 400 and n["agents"].tobytes() == end.tobytes()

"""The host side of the hyper-parameter sweep (hybridgl_amd/sweep.py, no GPU): the --sweep spec parser, the reduction of the
[C, n, 6] rows to per-configuration reports against a numpy restatement, and the exchange of a sharded sweep through
dist.gather_rows on CPU over gloo, world_size 2."""
import os
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hybridgl_amd import dist as D     # noqa: E402
from hybridgl_amd import sweep as SW   # noqa: E402

RUN = (0.5, 0.6, 3, 6)      # the run's own values: what an omitted axis keeps


def test_spec_lists_and_the_product_order():
    """r is the slowest axis, then alpha, k1, k2 the fastest -- whatever the order of the axes in the spec; values keep the
    order they were written in"""
    got = SW.parse_sweep_spec("k2=6,4;r=0.7,0.3;alpha=0.5;k1=3,2", *RUN)
    want = [(r, 0.5, k1, k2) for r in (0.7, 0.3) for k1 in (3, 2) for k2 in (6, 4)]
    assert got == want
    assert all(isinstance(t[0], float) and isinstance(t[1], float) and isinstance(t[2], int) and isinstance(t[3], int) for t in got)


def test_spec_ranges_and_the_endpoint_rule():
    got = SW.parse_sweep_spec("alpha=0:1:0.1", *RUN)
    assert len(got) == 11 and [t[1] for t in got] == [0 + i * 0.1 for i in range(11)] and got[-1][1] == 1.0
    assert all(t[0] == 0.5 and t[2:] == (3, 6) for t in got)
    # 0.1 + 2 * 0.1 = 0.30000000000000004 reaches 0.3 within 1e-9: included; 0.25 is not reached: the range ends at 0.2
    assert [t[0] for t in SW.parse_sweep_spec("r=0.1:0.3:0.1", *RUN)] == [0.1, 0.2, 0.1 + 2 * 0.1]
    assert [t[0] for t in SW.parse_sweep_spec("r=0.1:0.25:0.1", *RUN)] == [0.1, 0.2]
    assert [t[0] for t in SW.parse_sweep_spec("r=0.4:0.4:1", *RUN)] == [0.4]
    assert [t[2] for t in SW.parse_sweep_spec("k1=1:6:2", *RUN)] == [1, 3, 5]
    full = SW.parse_sweep_spec("r=0.3,0.5,0.7;alpha=0:1:0.1;k1=3;k2=6", *RUN)
    assert len(full) == 33 and full[0] == (0.3, 0.0, 3, 6) and full[11] == (0.5, 0.0, 3, 6) and full[-1] == (0.7, 1.0, 3, 6)


def test_spec_omitted_axes_keep_the_runs_values():
    assert SW.parse_sweep_spec("alpha=0.2", 0.25, 0.6, 2, 5) == [(0.25, 0.2, 2, 5)]
    assert SW.parse_sweep_spec("k2=4 ; ", 0.25, 0.6, 2, 5) == [(0.25, 0.6, 2, 4)]


@pytest.mark.parametrize("spec", ["", " ", ";", "alpha", "beta=1", "alpha=", "alpha=a", "alpha=0:1", "alpha=0:1:0", "alpha=1:0:0.1",
                                  "alpha=0:1:0.1:2", "k1=2.5", "k1=0", "k2=0:3:1", "alpha=0.1;alpha=0.2", "r=0.1,,0.2"])
def test_malformed_spec_raises(spec):
    with pytest.raises(ValueError, match="--sweep"):
        SW.parse_sweep_spec(spec, *RUN)


def _sweep_rows(C, positions, seed=0):
    """made-up rows of a sweep: rows [C, n, 6] and ceiling [n, 5] of the given dataset positions, two sentences each; one
    sentence with U = 0 under every configuration"""
    rng = np.random.default_rng(seed)
    owners = np.array([(p, s) for p in positions for s in range(2)], dtype=np.int64).reshape(-1, 2)
    n = len(owners)
    rows = np.zeros((C, n, 6), dtype=np.int64)
    ceil = np.zeros((n, 5), dtype=np.int64)
    for j, (p, s) in enumerate(owners):
        g = np.random.default_rng(1000 * int(p) + int(s) + seed)      # a sentence's numbers depend on the sentence alone
        U = g.integers(50, 500, 2 * C)
        I = (U * g.random(2 * C)).astype(np.int64)
        rows[:, j, 0:2] = (p, s)
        rows[:, j, 2], rows[:, j, 3], rows[:, j, 4], rows[:, j, 5] = I[:C], U[:C], I[C:], U[C:]
        ceil[j] = (p, s, g.integers(0, 64), U[0], U[0] + g.integers(0, 9))
        if p == 3 and s == 1:
            rows[:, j, 2:6] = 0
            ceil[j, 3:5] = 0
    del rng
    return rows, ceil


def test_metric_reduction_equals_a_numpy_restatement():
    C = 5
    rows, ceil = _sweep_rows(C, [4, 0, 3, 1])       # out of order: the report sorts by (position, sentence)
    configs = [(0.1 * c, 0.5, 3, 6) for c in range(C)]
    packed = SW.pack_rows(rows, ceil)
    assert packed.shape == (8 * (C + 1), 6) and packed.dtype == np.int64
    back, ceil6 = SW.unpack_rows(packed, C)
    assert np.array_equal(back, rows) and np.array_equal(ceil6[:, :2], ceil[:, :2]) and np.array_equal(ceil6[:, 2:4], ceil[:, 3:5])
    sm = SW.sweep_metrics_from_rows(back, ceil6, configs)
    order = np.lexsort((rows[0, :, 1], rows[0, :, 0]))

    def miou(i, u):      # Hybridgl_main.py:240-247: float32 I / U per sentence, 0 where U == 0, the mean times 100
        i, u = i[order].astype(np.float32), u[order].astype(np.float32)
        q = np.where(u == 0, np.float32(0), i / np.where(u == 0, np.float32(1), u)).astype(np.float32)
        return q

    import torch
    for c in range(C):
        m = sm["configs"][c]
        s = rows[c, :, 2:6].sum(0)
        assert m["cum"] == s.tolist() and m["n_sentences"] == 8
        assert m["oIoU"] == float(s[0]) * 100.0 / float(s[1]) and m["oIoU_final"] == float(s[2]) * 100.0 / float(s[3])
        assert m["mIoU"] == float(torch.mean(torch.from_numpy(miou(rows[c, :, 2], rows[c, :, 3]))) * 100.0)
        assert m["mIoU_final"] == float(torch.mean(torch.from_numpy(miou(rows[c, :, 4], rows[c, :, 5]))) * 100.0)
        assert (m["r"], m["alpha"], m["k1"], m["k2"]) == configs[c]
        assert {k: v for k, v in m.items() if k not in ("r", "alpha", "k1", "k2")} == D.metrics_from_rows(rows[c])
    cs = ceil[:, 3:5].sum(0)
    assert sm["ceiling"]["cum"] == cs.tolist() and sm["ceiling"]["oIoU"] == float(cs[0]) * 100.0 / float(cs[1])
    assert sm["ceiling"]["mIoU"] == float(torch.mean(torch.from_numpy(miou(ceil[:, 3], ceil[:, 4]))) * 100.0)
    assert sm["best"] == int(np.argmax([rows[c, :, 4].sum() / rows[c, :, 5].sum() for c in range(C)]))
    # the first of equal maxima
    twice = np.concatenate([rows, rows[sm["best"]:sm["best"] + 1]], axis=0)
    assert SW.sweep_metrics_from_rows(twice, ceil6)["best"] == sm["best"]
    empty = SW.sweep_metrics_from_rows(np.zeros((2, 0, 6), np.int64), np.zeros((0, 6), np.int64))
    assert empty["best"] == 0 and empty["ceiling"]["oIoU"] == 0.0 and empty["configs"][1]["n_sentences"] == 0


def _worker(rank, world, port, n_items, C, q):
    os.environ.update({"RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": str(world),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    sys.path.insert(0, ROOT)
    from hybridgl_amd import dist as DD
    from hybridgl_amd import sweep as SS
    dist = DD.init_process_group("gloo")
    r, _, w = DD.env_rank()
    rows, ceil = _sweep_rows(C, DD.shard_indices(n_items, r, w))       # this rank's strided half
    packed = DD.gather_rows(SS.pack_rows(rows, ceil), dist)
    back, ceil6 = SS.unpack_rows(packed, C)
    dist.barrier()
    q.put((rank, SS.sweep_metrics_from_rows(back, ceil6), back.shape, rows.shape[1]))
    dist.destroy_process_group()


def test_two_ranks_gather_the_sweep_rows_through_gather_rows():
    """each rank holds the rows of its strided share of 5 items (6 and 4 sentences); after ONE dist.gather_rows exchange of the
    packed rows every rank reports what a single process reports"""
    n_items, world, C = 5, 2, 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = D.free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_items, C, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    rows, ceil = _sweep_rows(C, range(n_items))
    single = SW.sweep_metrics_from_rows(*SW.unpack_rows(SW.pack_rows(rows, ceil), C))
    for rank, sm, shape, n_own in got:
        assert sm == single, (rank, sm, single)
        assert shape == (C, 10, 6)
    assert [g[3] for g in got] == [6, 4]


def test_driver_flags_and_report_shape():
    from hybridgl_amd import main as drv
    args = drv.default_argument_parser().parse_args(["--sweep", "alpha=0:1:0.5", "--sweep_json", "out.json"])
    assert args.sweep == "alpha=0:1:0.5" and args.sweep_json == "out.json"
    assert drv.default_argument_parser().parse_args([]).sweep == ""
    rows, ceil = _sweep_rows(3, [0, 1])
    configs = SW.parse_sweep_spec(args.sweep, *RUN)
    sm = SW.sweep_metrics_from_rows(*SW.unpack_rows(SW.pack_rows(rows, ceil), 3), configs)
    rep = drv.sweep_report(configs, sm)
    assert rep["configs"] == [dict(r=0.5, alpha=a, k1=3, k2=6) for a in (0.0, 0.5, 1.0)]
    assert [set(m) for m in rep["metrics"]] == [{"r", "alpha", "k1", "k2", "oIoU", "mIoU", "oIoU_final", "mIoU_final", "n_sentences"}] * 3
    assert rep["best"]["index"] == sm["best"] and rep["best"]["oIoU_final"] == max(m["oIoU_final"] for m in rep["metrics"])
    assert set(rep["ceiling"]) == {"oIoU", "mIoU", "cum", "n_sentences"}
    import json
    json.dumps(rep)

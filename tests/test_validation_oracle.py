"""Validation pass, host arithmetic against tests/_oracle_validation.py: the scalar writer, and the data-parallel
combination of the per-rank (sum, count) pairs in rank order over a gloo group of 2."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _oracle_validation as OV
from onetrainer_amd.trainer.validation import gather_ranks, validation_scalars


def _losses(n, seed):
    rng = np.random.default_rng(seed)
    return (10.0 ** rng.uniform(-6, 3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def test_oracle_accumulate_is_the_sequential_double_sum():
    losses = _losses(50, 0)
    idx = np.random.default_rng(1).integers(0, 3, 50)
    acc = OV.accumulate(np.zeros((4, 2)), losses, idx)
    for c in range(4):
        s = 0.0
        for v in losses[idx == c]:
            s += float(v)
        assert acc[c, 0] == s and acc[c, 1] == (idx == c).sum()
    before = acc.copy()
    OV.accumulate(acc, [1.0, 2.0], [-1, 4])   # outside [0, n): skipped
    assert (acc == before).all()


def test_scalar_writer_matches_the_reference_arithmetic():
    concepts = [{"name": "x", "path": "/p/a", "seed": 1}, {"name": "x", "path": "/p/b", "seed": 2},
                {"name": "", "path": "/p/dogs", "seed": 3}, {"name": "x", "path": "/p/c", "seed": 1},
                {"name": "empty", "path": "/p/e", "seed": 9}]
    acc = np.zeros((5, 2))
    OV.accumulate(acc, _losses(40, 2), np.random.default_rng(3).integers(0, 4, 40))   # concept 4 gets no sample
    got = validation_scalars(torch.from_numpy(acc), concepts)
    exp = OV.scalars(acc.tolist(), concepts)
    assert got == exp                                          # same tags, same order, the same float64 bits
    assert [t for t, _ in got] == ["loss/validation_step/x", "loss/validation_step/x(1)",
                                   "loss/validation_step/dogs", "loss/validation_step/total_average"]
    assert got[0][1] == (acc[0, 0] + acc[3, 0]) / (acc[0, 1] + acc[3, 1])   # one seed: merged in index order
    # one seed with samples: no total average
    one = validation_scalars([[3.0, 2.0], [0.0, 0.0]], concepts[:2])
    assert one == [("loss/validation_step/x", 1.5)] == OV.scalars([[3.0, 2.0], [0.0, 0.0]], concepts[:2])
    assert validation_scalars([[0.0, 0.0]], concepts[:1]) == []


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_acc(rank):
    acc = np.zeros((3, 2))
    OV.accumulate(acc, _losses(17 + rank, 10 + rank), np.random.default_rng(20 + rank).integers(0, 3, 17 + rank))
    return acc


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        total = gather_ranks(torch.from_numpy(_rank_acc(rank)), world)
        q.put((rank, total.tolist()))
    except Exception as e:  # pragma: no cover
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def test_rank_order_combination_gloo_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    exp = (_rank_acc(0) + _rank_acc(1)).tolist()   # rank 0 first, then rank 1
    assert res == {0: exp, 1: exp}, res
    assert gather_ranks(torch.ones(2, 2), 1).tolist() == [[1.0, 1.0], [1.0, 1.0]]   # one process: untouched

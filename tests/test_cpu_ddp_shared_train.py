"""A gloo world-2 dry run of the data-parallel wrapper's tuning broadcast for SHARED TRAINING batches (the model is
tests/test_cpu_host.py::test_ddp_tuning_sync_is_rank_symmetric_gloo_world2): the grouped training loader gives every rank the same
(Bi, Q), so the broadcast is keyed on (Bi, Q, H, W, training, ...) and both ranks must issue the same collectives whatever
query-length bucket each of them meets first.  A mismatch would hang or raise inside mp.spawn."""
import os
import socket

import torch
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from zsgnet_pytorch_amd import ops
    from zsgnet_pytorch_amd.dist import DistributedDataParallel
    dist.init_process_group("gloo", rank=rank, world_size=world)

    class Store:
        pass

    class Fake(torch.nn.Module):
        """the attributes of ZSGNet the wrapper touches, shared-training opt-in included"""

        def __init__(self):
            super().__init__()
            self.store = Store()
            self.store.flat, self.store.grad = torch.zeros(8), torch.zeros(8)
            self._rmv = torch.zeros(8)
            self._nbt = torch.tensor([0])
            self._plans, self.lowered = {}, []
            self._shared_train = True

        def plan_geometry(self, inp):
            T = 20 if inp["qvec"].shape[1] <= 20 else 50
            if inp.get("img_idx") is not None:
                return (inp["img"].shape[0], inp["qvec"].shape[0], 96, 96, T)
            return (inp["qvec"].shape[0], 96, 96, T)

        def _plan_for(self, B, H, W, T, Q=None):
            self.lowered.append((B, Q, T))
            ops._TUNE_CACHE[("fake", B, Q, H, W, T)] = 7          # "rank 0 tuned something"

        def forward(self, inp):
            return inp["qvec"].sum()
    m = Fake().train()
    ddp = DistributedDataParallel(m)

    def batch(Bi, Q, T):
        return {"img": torch.zeros(Bi, 3, 8, 8), "qvec": torch.zeros(Q, T, 4), "img_idx": torch.arange(Q) % Bi}
    # step:        0   1   2   3          (rank 1 meets bucket 50 two steps before rank 0 does)
    lens = [[12, 18, 31, 40], [33, 15, 9, 44]][rank]
    for T in lens:
        ddp(batch(2, 8, T))
        x = torch.ones(1)
        dist.all_reduce(x)                                     # the step's gradient collective: must pair up on both ranks
        assert float(x) == world
    n_one = len(ddp._tuned)
    ddp(batch(4, 8, lens[0]))                                  # another (Bi, Q): a new, symmetric key
    ddp({"qvec": torch.zeros(8, lens[1], 4)})                  # a plain batch of the same size: its own key
    n_three = len(ddp._tuned)
    m.eval()
    ddp(batch(2, 8, lens[0]))                                  # eval-mode shared batches: no broadcast at all
    x = torch.ones(1)
    dist.all_reduce(x)
    ret[rank] = (n_one, n_three, len(ddp._tuned), dict(ops._TUNE_CACHE), list(m.lowered))
    dist.barrier()
    dist.destroy_process_group()


def test_shared_training_tuning_sync_is_rank_symmetric_gloo_world2():
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    for r in (0, 1):
        assert ret[r][0] == 1, "one broadcast per (Bi, Q, H, W, mode), not per query-length bucket"
        assert ret[r][1] == 3 and ret[r][2] == 3, "a new (Bi, Q) and a plain batch are new keys; an eval-mode shared batch is none"
    assert ret[0][4] == [(2, 8, 20), (4, 8, 20), (8, None, 20)] and ret[1][4] == [], "only rank 0 lowers ahead of the broadcast (its own bucket)"
    assert ret[1][3] == ret[0][3] and ret[0][3], "rank 1 runs rank 0's table"

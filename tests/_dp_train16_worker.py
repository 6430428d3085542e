"""Worker of tests/test_gpu_rdt_dp_fp16.py: one of two ranks sharing cuda:0 over gloo, fine-tuning in fp16 with a loss scale.

    python -m tests._dp_train16_worker <rank> <port>

The overflow check runs on the all-reduced arena: a non-finite value on one rank is non-finite in the sum on every rank, so both ranks take
the same branch without another collective.  One `DP_OK <scenario>` line each; helpers and failure handling are tests/_dp_train_worker.py's."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vla-touch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch
import torch.distributed as dist

from tests._dp_train_worker import SEEDS, TIMEOUT, _digest, _gathered, _loss_and_fold, _mk, _run, _state, _step


def main(rank: int, port: str) -> None:
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    torch.set_grad_enabled(False)
    dist.init_process_group("gloo", rank=rank, world_size=2, timeout=TIMEOUT)
    G, W = dist.group.WORLD, 2
    from tests import cases
    from tests import rdt_train_ref as R
    cfg = cases.RDT_TINY
    sd = cases.rdt_sd(cfg)
    batches = [R.batch(cfg, 3, 12, seed=s) for s in SEEDS[:4]]
    bad = dict(batches[1])
    bad["action_gt"] = batches[1]["action_gt"].clone()
    bad["action_gt"][0, 0, 0] = float("inf")

    def skip(comm_dtype):
        def run():
            dp = _mk(cfg, sd, process_group=G, precision="fp16", loss_scale=dict(init_scale=1024.0, growth_interval=1), lr=1e-3, comm_dtype=comm_dtype)
            start = _digest(dp.p.values())
            loss = float(_step(dp, bad if rank == 1 else batches[0]))            # rank 1 alone sees the inf
            assert (loss == loss and abs(loss) != float("inf")) == (rank == 0)
            assert dp.last_step_skipped and (dp.step_count, dp.skipped_steps, dp.global_step, dp.loss_scale_value) == (0, 1, 1, 512.0)
            assert dp.skipped_nonfinite_loss == (1 if rank == 1 else 0)          # each rank reads its own last loss
            assert _digest(dp.p.values()) == start
            assert float(_step(dp, batches[2 + rank])) > 0 and not dp.last_step_skipped
            assert (dp.step_count, dp.global_step, dp.loss_scale_value, dp.growth_tracker) == (1, 2, 1024.0, 0)
            got = _gathered((_state(dp), dp.loss_scale_value, dp.skipped_steps, dp.step_count), G)
            assert got[0] == got[1], "the two ranks differ after a skipped and a clean step"
            return f"norm {float(dp.grad_norm):.6f}"
        return run

    def exact():
        kw = dict(precision="fp16", loss_scale=1024.0, lr=1e-3)
        dp, one = _mk(cfg, sd, process_group=G, **kw), _mk(cfg, sd, gradient_accumulation_steps=2, **kw)
        _step(dp, batches[rank])
        for b in batches[:W]:
            _loss_and_fold(one, b)
        one.optimizer_step()
        assert not dp.last_step_skipped and not one.last_step_skipped and dp.global_step == one.global_step == 1
        a, b_ = _state(dp), _state(one)
        assert a == b_, ("the grouped fp16 trainer differs from one process with k = 2 in", [k for k in a if a[k] != b_[k]])
        states = _gathered(a, G)
        assert states[0] == states[1], "the two ranks differ"
        return f"norm {float(dp.grad_norm):.6f}"

    def disagreement():
        import pytest
        with pytest.raises(ValueError, match="loss_scale"):
            _mk(cfg, sd, process_group=G, precision="fp16", loss_scale=(1024.0, 2048.0)[rank])

    for name, fn in (("skip_fp32_exchange", skip("fp32")), ("skip_bf16_exchange", skip("bf16")), ("exact_k2", exact), ("disagreement", disagreement)):
        _run(name, fn)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(int(sys.argv[1]), sys.argv[2])

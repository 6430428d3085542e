"""Worker of tests/test_rdt_dp_host.py and tests/test_gpu_rdt_dp.py: one rank of a data-parallel RDT fine-tuning run.

    python -m tests._dp_train_worker hostsum <rank> <port> <out>      two CPU ranks over gloo: all-reduce bf16 tensors, rank 0 saves the sum
    python -m tests._dp_train_worker gloo <rank> <port> <tmpdir>      two ranks sharing cuda:0 over gloo (RCCL refuses two ranks on one device):
                                                                      every two-rank scenario, one `DP_OK <scenario>` line each
    python -m tests._dp_train_worker nccl <port>                      one rank over "nccl" (= RCCL), world size 1: the production collectives

Every rank also runs the one-process comparison trainer itself, so nothing but small digests and the gathered gradients travels between the
ranks for the checks.  A failed scenario prints its traceback and ends the process at once: the other rank's next collective then fails
instead of waiting, and the parent kills both on its time limit anyway.  init_process_group gets timeout = 120 s, so a lone rank errors."""
import datetime
import hashlib
import json
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vla-touch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch
import torch.distributed as dist

TIMEOUT = datetime.timedelta(seconds=120)
SEEDS = (6, 16, 26, 36, 46, 56, 66, 76)
DEV = "cuda:0"


def hostsum(rank: int, port: str, out: str) -> None:
    """200 000 mixed-magnitude values per rank, rounded to bf16 on the host and summed by gloo."""
    from tests import rdt_dp_ref as P
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    dist.init_process_group("gloo", rank=rank, world_size=2, timeout=TIMEOUT)
    t = P.bf16_rne(P.mixed_values(200_000, 500 + rank))
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    if rank == 0:
        torch.save(t, out)
    dist.barrier()
    dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ helpers of the GPU modes
def _digest(tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _state(tr) -> dict:
    """Digests of everything a step changes: parameters, moments (codes and scales under adamw8bit), shadows, and the norm."""
    d = {"p": _digest(tr.p.values()), "shadow": _digest(tr.shadow[k] for k in tr.p), "norm": _digest([tr._norm_coef[:1]])}
    for name in ("_m", "_v", "_am", "_av"):
        store = getattr(tr, name)
        d[name] = _digest(store[k] for k in sorted(store))
    return d


def _gathered(obj, group):
    got = [None] * dist.get_world_size(group)
    dist.all_gather_object(got, obj, group=group)
    return got


def _mk(cfg, sd, **kw):
    from vlatouch.rdt_train import RdtTrainer
    return RdtTrainer(sd, heads=cfg["heads"], horizon=cfg["horizon"], action_dim=cfg["action_dim"], device=DEV, **kw)


def _args(b):
    return (b["lang_tokens"], b["lang_attn_mask"], b["img_tokens"], b["state_tokens"], b["action_gt"], b["action_mask"], b["ctrl_freqs"])


def _step(tr, b):
    return tr.train_step(*_args(b), noise=b["noise"], timesteps=b["timesteps"])


def _loss_and_fold(tr, b):
    tr.get_loss(*_args(b), noise=b["noise"], timesteps=b["timesteps"])
    fresh = {k: tr.g[k].detach().reshape(tr.p[k].shape).cpu().clone() for k in tr.p}
    tr.accumulate()
    return fresh


def _run(name, fn):
    try:
        info = fn()
        torch.cuda.synchronize()
        print(f"DP_OK {name} {info or ''}", flush=True)
    except BaseException:
        traceback.print_exc()
        print(f"DP_FAIL {name}", flush=True)
        sys.stdout.flush(), sys.stderr.flush()
        os._exit(1)


# ------------------------------------------------------------------------------------------------ two ranks on cuda:0 over gloo
def gloo(rank: int, port: str, tmpdir: str) -> None:
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    torch.set_grad_enabled(False)
    dist.init_process_group("gloo", rank=rank, world_size=2, timeout=TIMEOUT)
    G, W = dist.group.WORLD, 2
    from tests import cases
    from tests import rdt_dp_ref as P
    from tests import rdt_train_ref as R
    from vlatouch import train as T
    cfg = cases.RDT_TINY
    sd = cases.rdt_sd(cfg)
    batches = [R.batch(cfg, 3, 12, seed=s) for s in SEEDS]
    mine = lambda n: [batches[W * i + rank] for i in range(n)]         # the round-robin of EpisodeStore.batches(rank=, world_size=)

    def broadcast():
        start = {k: v * 0.5 for k, v in sd.items()} if rank == 1 else sd
        tr = _mk(cfg, start, process_group=G)
        got = _gathered(_digest(tr.p.values()), G)
        want = _digest(v.to(torch.float32) for v in sd.values())
        assert _digest(start.values()) != want or rank == 0, "rank 1 must start from other weights"
        assert got == [want, want], "after construction every rank holds rank 0's parameters, bit for bit"
        assert (tr.world, tr.rank) == (2, rank)

    def disagreement():
        import pytest
        with pytest.raises(ValueError, match="gradient_accumulation_steps"):
            _mk(cfg, sd, process_group=G, gradient_accumulation_steps=1 + rank)
        with pytest.raises(ValueError, match="comm_dtype"):
            _mk(cfg, sd, process_group=G, comm_dtype=("fp32", "bf16")[rank])

    def exact(optimizer, steps):
        def run():
            chunks = sum((v.numel() + T.MT_CHUNK - 1) // T.MT_CHUNK for v in sd.values())
            assert chunks > 3 and chunks % 3 != 0, "the buckets must split and the last one must be ragged"
            kw = dict(lr=1e-3, optimizer=optimizer)
            dp = _mk(cfg, sd, process_group=G, comm_bucket_bytes=3 * T.MT_CHUNK * 4, **kw)
            one = _mk(cfg, sd, gradient_accumulation_steps=2, **kw)
            losses = [float(_step(dp, b)) for b in mine(steps)]
            assert dp.global_step == steps and dp.sync_gradients and dp.micro_step == 0
            # The comparison trainer is driven by get_loss / accumulate / optimizer_step, not by train_step: train_step moves the EMA on every
            # micro-batch (EMAModel.step once per loop iteration), which a one-process loop passes twice per optimizer step and each of the
            # two ranks once.  Driven like this it takes one EMA update per optimizer step, as each rank does, and the shadows are comparable.
            for i in range(steps):
                for b in batches[W * i:W * i + W]:
                    _loss_and_fold(one, b)
                one.optimizer_step()
            assert one.global_step == steps and one.ema_updates == dp.ema_updates == steps
            a, b_ = _state(dp), _state(one)
            assert a == b_, ("the grouped trainer differs from one process with k = 2 in", [k for k in a if a[k] != b_[k]])
            states = _gathered(a, G)
            assert states[0] == states[1], "the two ranks differ"
            all_losses = _gathered(losses, G)
            assert all(x != y for x, y in zip(*all_losses)), ("the ranks' local losses must differ, or the test shows nothing", all_losses)
            return f"norm {float(dp.grad_norm):.6f} losses {all_losses}"
        return run

    def accumulated():
        dp = _mk(cfg, sd, process_group=G, gradient_accumulation_steps=2, lr=1e-3)
        one = _mk(cfg, sd, gradient_accumulation_steps=4, lr=1e-3)
        for b in mine(2):
            _loss_and_fold(dp, b)
        fresh = [_loss_and_fold(one, b) for b in batches[:4]]
        got, worst = dp.grads(), 0.0
        for k in sd:
            ref = sum(f[k].double() for f in fresh) / 4
            mag = sum(f[k].double().abs() for f in fresh) / 4
            err = (got[k].double() - ref).abs()
            bound = 4 * 2.0 ** -23 * mag
            assert bool((err <= bound).all()), (k, float((err - bound).max()))
            nz = mag > 0
            if bool(nz.any()):
                worst = max(worst, float((err[nz] / mag[nz]).max()))
        dp.optimizer_step(), one.optimizer_step()
        n_dp, n_one = float(dp.grad_norm), float(one.grad_norm)
        assert abs(n_dp - n_one) <= 1e-5 * n_one, (n_dp, n_one)
        states = _gathered(_state(dp), G)
        assert states[0] == states[1], "the two ranks differ after the step"
        return f"worst element {worst / 2.0 ** -23:.3f} x 2^-23 of sum|g|/4 (bar 4); norm {n_dp:.7f} vs {n_one:.7f}"

    def bf16_exchange():
        sd16 = R.round_bf16(sd)
        dp = _mk(cfg, sd16, process_group=G, comm_dtype="bf16", precision="bf16")
        fresh = _loss_and_fold(dp, R.round_bf16(batches[rank]))
        got = dp.grads()
        local = _gathered(fresh, G)
        differ = 0
        for k in sd:
            want = P.bf16_exchange(local[0][k] * 0.5, local[1][k] * 0.5).float()
            assert got[k].view(torch.int32).equal(want.view(torch.int32)), (k, float((got[k] - want).abs().max()))
            differ += int((want != (local[0][k] * 0.5 + local[1][k] * 0.5)).sum())
        assert differ > 0, "the bf16 exchange must differ from the fp32 sum somewhere, or the test shows nothing"
        return f"{differ} elements differ from the fp32 sum"

    def resume():
        from tests.test_gpu_rdt_train import _runner
        from vlatouch.rdt_train import finetune
        out = os.path.join(tmpdir, "run")
        kw = dict(process_group=G, lr=1e-3)
        straight = _runner(cfg).trainer(**kw)
        finetune(straight, mine(4), max_train_steps=4)
        first = _runner(cfg).trainer(**kw)
        finetune(first, mine(4), max_train_steps=2, checkpointing_period=2, output_dir=out)
        assert first.global_step == 2
        assert sorted(d for d in os.listdir(out) if d.startswith("checkpoint")) == ["checkpoint-2"]
        second = _runner(cfg).trainer(**kw)
        finetune(second, mine(4)[2:], max_train_steps=4, checkpointing_period=2, output_dir=out, resume_from_checkpoint="latest")
        assert second.global_step == 4
        assert sorted(os.listdir(out)) == ["checkpoint-2", "checkpoint-4", "config.json", "ema", "model.safetensors"], os.listdir(out)
        assert sorted(os.listdir(os.path.join(out, "checkpoint-4"))) == ["checkpoint", "ema", "trainer_state.json"]
        with open(os.path.join(out, "checkpoint-4", "trainer_state.json")) as f:
            st = json.load(f)
        assert st["world_size"] == 2 and st["comm_dtype"] == "fp32" and st["global_step"] == 4
        a, b_ = _state(straight), _state(second)
        assert a == b_, ("the resumed run differs from the straight one in", [k for k in a if a[k] != b_[k]])
        states = _gathered(b_, G)
        assert states[0] == states[1]

    def evaluation():
        import types
        from tests import sample_eval_ref as S
        from tests.test_gpu_sample_eval import ID2NAME, _runner
        from train.sample import log_sample_res
        from vlatouch.rdt_train import sample_eval, sample_eval_means, sample_eval_sums
        runner = _runner(cfg)
        local = [S.collator_batch(cfg, 3, 12, 300 + 10 * (W * j + rank), S.G18_INDICES[(j + rank) % 2]) for j in range(2)]
        acc, count, keys = sample_eval_sums(runner, local, num_sample_batches=2, dataset_id2name=ID2NAME)
        parts = _gathered((acc, count, dict(keys)), G)
        assert not torch.equal(parts[0][0], parts[1][0]), "the two ranks must evaluate different batches"
        total, counts, union = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1], {**parts[0][2], **parts[1][2]}
        want = sample_eval_means(total, counts, union, 2 * W)
        metrics, raw = sample_eval(runner, local, num_sample_batches=2, dataset_id2name=ID2NAME, return_raw=True, group=G)
        assert raw == want, (raw, want)
        assert metrics == {k: round(v, 4) for k, v in want.items()}
        alone = sample_eval_means(acc, count, keys, 2)
        assert alone["overall_avg_sample_mse"] != raw["overall_avg_sample_mse"]
        args = types.SimpleNamespace(num_sample_batches=2, precomp_lang_embed=True)
        assert log_sample_res(None, None, runner, args, types.SimpleNamespace(process_group=G), torch.float32, ID2NAME, local, None) == metrics
        return json.dumps(metrics)

    for name, fn in (("broadcast", broadcast), ("disagreement", disagreement), ("exact_adamw", exact("adamw", 3)),
                     ("exact_adamw8bit", exact("adamw8bit", 1)), ("accumulated", accumulated), ("bf16_exchange", bf16_exchange),
                     ("resume", resume), ("evaluation", evaluation)):
        _run(name, fn)
    dist.barrier()
    dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ RCCL itself, world size 1
def nccl(port: str) -> None:
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK="0", WORLD_SIZE="1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev, timeout=TIMEOUT)
    assert dist.get_backend() == "nccl"
    G = dist.group.WORLD
    from tests import cases
    from tests import rdt_train_ref as R
    from vlatouch import train as T
    cfg = cases.RDT_TINY
    sd = cases.rdt_sd(cfg)
    batches = [R.batch(cfg, 3, 12, seed=s) for s in SEEDS[:4]]

    def fp32_exchange():
        for k in (1, 2):
            kw = dict(lr=1e-3, gradient_accumulation_steps=k)
            dp, one = _mk(cfg, sd, process_group=G, comm_bucket_bytes=3 * T.MT_CHUNK * 4, **kw), _mk(cfg, sd, **kw)
            for b in batches[:2 * k]:
                la, lb = _step(dp, b), _step(one, b)
                assert torch.equal(la, lb)
            assert dp.global_step == one.global_step == 2
            a, b_ = _state(dp), _state(one)
            assert a == b_, (k, [n for n in a if a[n] != b_[n]])

    def bf16_exchange():
        sd16, b = R.round_bf16(sd), R.round_bf16(batches[0])
        dp, one = _mk(cfg, sd16, process_group=G, comm_dtype="bf16", precision="bf16"), _mk(cfg, sd16, precision="bf16")
        _loss_and_fold(dp, b)
        one.get_loss(*_args(b), noise=b["noise"], timesteps=b["timesteps"])
        got, ref = dp.grads(), one.grads()
        differ = 0
        for k in sd:
            want = ref[k].to(torch.bfloat16).float()
            assert got[k].view(torch.int32).equal(want.view(torch.int32)), k
            differ += int((want != ref[k]).sum())
        assert differ > 0
        dp.optimizer_step()
        assert bool(torch.isfinite(dp.grad_norm))

    _run("nccl_fp32_exchange", fp32_exchange)
    _run("nccl_bf16_exchange", bf16_exchange)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "hostsum":
        hostsum(int(sys.argv[2]), sys.argv[3], sys.argv[4])
    elif mode == "gloo":
        gloo(int(sys.argv[2]), sys.argv[3], sys.argv[4])
    elif mode == "nccl":
        nccl(sys.argv[2])
    else:
        raise SystemExit(f"unknown mode {mode!r}")

"""Two saved bf16 cases of the RDT training kernels that gained an fp16 instantiation (csrc/vt_train_rdt.hip, csrc/vt_attn_bwd.hip): seeded
inputs, the calls, and one sha256 digest per output.  tests/golden/g20_bf16_train_kernels.json holds the digests a build of the commit BEFORE
the fp16 mode gave on an MI355X (tools/make_golden_bf16_train.py wrote it, run against that commit's library); the fp16 kernel test recomputes
them, so templating the kernels on the 16-bit type is shown to have left every bf16 bit where it was.  Only calls that commit already had.

A second set, `parent_cases` (tests/golden/g22_train_kernels_parent.json), was recorded the same way at the commit BEFORE the kernels' dtype
dispatch and chunk walk were each stated once (DISPATCH_T in csrc/vt_common.h, mt_chunk / mt_walk in csrc/vt_optim.h): the fp32 and fp16
instantiations of the same calls, the entry points the Python wrappers never reach with fp32, vt_sample_metrics, and the eight
multi-tensor table kernels on aligned and unaligned tensors, guard words included."""
import ctypes as C
import hashlib
from collections import OrderedDict

import torch

BF, H16, F32 = torch.bfloat16, torch.float16, torch.float32
GOLDEN_NAME = "g20_bf16_train_kernels.json"
PARENT_GOLDEN_NAME = "g22_train_kernels_parent.json"


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _elementwise(dev, dt=BF) -> "OrderedDict[str, torch.Tensor]":
    """dt: the activation dtype of the case (the saved bf16 case by default)."""
    from vlatouch import _lib as L
    from vlatouch import rdt_train as RT
    g = torch.Generator().manual_seed(20)
    r = lambda *shape: torch.randn(*shape, generator=g)
    out = OrderedDict()
    x, w, dy = (r(5, 256) * 1.7 + 0.3).to(dev, dt), (1 + 0.2 * r(256)).to(dev), r(5, 256).to(dev, dt)
    out["rmsnorm.dx"], out["rmsnorm.dw"] = RT.rmsnorm_bwd(x, w, dy, 1e-6, L.NORM_RMS_MEANSQ)
    out["rmsnorm_var.dx"], out["rmsnorm_var.dw"] = RT.rmsnorm_bwd(x, w, dy, 1e-6, L.NORM_RMS_VAR)
    buf, hw, dbuf = (r(33, 768) * 1.3 + 0.2).to(dev, dt), (1 + 0.2 * r(64)).to(dev), r(33, 768).to(dev, dt)
    out["headnorm.dw"] = RT.headnorm_bwd_(buf[:, 256:512], dbuf[:, 256:512], 4, hw, 1e-6, L.NORM_RMS_VAR)      # 132 pairs: a ragged last group of 64
    out["headnorm.dx"] = dbuf
    a = (r(1000) * 3).to(dev, dt)
    out["gelu"], out["gelu.d"] = RT.act(a, L.ACT_GELU_TANH), RT.act(a, L.ACT_GELU_TANH, r(1000).to(dev, dt))
    out["silu"], out["silu.d"] = RT.act(a, L.ACT_SILU), RT.act(a, L.ACT_SILU, r(1000).to(dev, dt))
    state, action, noise, mask = r(3, 1, 16).to(dev), r(3, 8, 16).to(dev), r(3, 8, 16).to(dev), (r(3, 1, 16) > 0).float().to(dev)
    ts = torch.tensor([3, 437, 998]).to(dev)
    out["qsample"] = RT.ddpm_qsample(state, action, noise, mask, ts, RT.alphas_cumprod(1000, "squaredcos_cap_v2").to(dev), dt)
    out["timestep_embed"] = RT.timestep_embed(ts.float(), RT.timestep_freqs(256).to(dev), dt)
    m = r(33, 40).to(dev, dt)
    pos = r(40).to(dev)
    av = m.clone()
    RT.add_rowvec_(av, pos)
    out["add_rowvec"] = av
    out["transpose_pad"], out["colsum"] = RT.transpose_pad(m), RT.colsum(m)
    out["add"] = RT.add_(m.clone(), r(33, 40).to(dev, dt))
    d = torch.zeros(33, 64, dtype=dt, device=dev)
    RT.copy_cols(m, 7, d, 13, 23)
    out["copy_cols"] = d
    out["mse.loss"], out["mse.dpred"] = RT.mse_loss(m, r(33, 40).to(dev))
    return out


def _attention(dev, dt=BF, only=None) -> "OrderedDict[str, torch.Tensor]":
    """only: the (shape tag, kernel) pairs to run; all four by default."""
    from vlatouch.rdt_train import attention_bwd
    out = OrderedDict()
    for tag, (B, Nq, Nk, H, masked) in (("67x20", (2, 67, 20, 4, True)), ("128x257", (2, 128, 257, 3, False))):
        g = torch.Generator().manual_seed(Nk)
        qb, kvb = torch.randn(B, Nq, H * 64, generator=g).to(dev, dt), torch.randn(B, Nk, 2 * H * 64, generator=g).to(dev, dt)
        do = torch.randn(B, Nq, H, 64, generator=g).to(dev, dt)
        km = None
        if masked:
            mask = torch.ones(B, Nk, dtype=torch.bool)
            mask[0, Nk - 3:] = False
            mask[1, :] = False
            km = mask.to(dev).to(torch.uint8).contiguous()
        q, k, v = qb.view(B, Nq, H, 64), kvb.view(B, Nk, 2, H, 64)[:, :, 0], kvb.view(B, Nk, 2, H, 64)[:, :, 1]
        for kernel in ("wave", "mfma"):
            if only is not None and (tag, kernel) not in only:
                continue
            dq, dkv = torch.zeros_like(qb), torch.zeros_like(kvb)
            ws = attention_bwd(q, k, v, do, dq.view(B, Nq, H, 64), dkv.view(B, Nk, 2, H, 64)[:, :, 0], dkv.view(B, Nk, 2, H, 64)[:, :, 1], kmask=km,
                               kernel=kernel)
            out[f"attn.{tag}.{kernel}.dq"], out[f"attn.{tag}.{kernel}.dkv"], out[f"attn.{tag}.{kernel}.ws"] = dq, dkv, ws
    return out


def bf16_saved_cases(dev) -> "OrderedDict[str, str]":
    """name -> sha256 of the output's bytes, for the element-wise case and the attention case."""
    out = OrderedDict()
    for part in (_elementwise(dev), _attention(dev)):
        torch.cuda.synchronize()
        for k, t in part.items():
            out[k] = digest(t)
    return out


# ------------------------------------------------------------------------------------------------ the second set (g22)
MT_SIZES = (1, 5, 4095, 4096, 4097, 3 * 4096 + 5)          # one element, a ragged tail that is no multiple of 4, the chunk boundary from both sides
SENTINEL, GUARD = 12345.0, 8


def _elementwise_direct(dev) -> "OrderedDict[str, torch.Tensor]":
    """vt_mse_loss_scaled in the three dtypes, and the typed column sum / add / column copy called with dt = fp32, which the wrappers of
    vlatouch.rdt_train never do (they take vt_train.hip's fp32 kernels)."""
    from vlatouch import _lib as L
    from vlatouch import rdt_train as RT
    g = torch.Generator().manual_seed(22)
    r = lambda *shape: torch.randn(*shape, generator=g)
    out = OrderedDict()
    m, tgt, b = r(33, 40), r(33, 40).to(dev), r(33, 40).to(dev)
    for tag, dt in (("fp32", F32), ("bf16", BF), ("fp16", H16)):
        out[f"mse_scaled.{tag}.loss"], out[f"mse_scaled.{tag}.dpred"] = RT.mse_loss(m.to(dev, dt), tgt, 3000.0)
    lib, sp, x = L.lib(), L.stream_ptr(torch.device(dev)), m.to(dev)
    cs = torch.full((40,), float("nan"), device=dev)
    L.check(lib.vt_colsum_dt(L.ptr(x), L.F32, 40, L.ptr(cs), 33, 40, sp), "vt_colsum_dt")
    a = x.clone()
    L.check(lib.vt_add_dt(L.ptr(a), L.ptr(b), a.numel(), L.F32, sp), "vt_add_dt")
    d = torch.zeros(33, 64, device=dev)
    L.check(lib.vt_copy_cols_dt(L.ptr(x), 40, 7, L.ptr(d), 64, 13, 33, 23, L.F32, sp), "vt_copy_cols_dt")
    out["colsum_dt.fp32"], out["add_dt.fp32"], out["copy_cols_dt.fp32"] = cs, a, d
    return out


def _sample_metrics(dev) -> "OrderedDict[str, torch.Tensor]":
    """vt_sample_metrics, B = 3, H = 4, A = 5, two datasets, twice into the same sums, pred in each dtype."""
    from vlatouch import _lib as L
    B, H, A, n = 3, 4, 5, 2
    g = torch.Generator().manual_seed(18)
    pred, tgt = torch.randn(B, H, A, generator=g), torch.randn(B, H, A, generator=g).to(dev)
    mask, sn = (torch.rand(B, A, generator=g) > 0.3).float().to(dev), (torch.rand(B, A, generator=g) + 0.1).to(dev)
    rows = torch.tensor([1, 0, 1], dtype=torch.int32).to(dev)
    out = OrderedDict()
    for tag, dt in (("fp32", F32), ("bf16", BF), ("fp16", H16)):
        res = torch.full((2 * B + 2,), float("nan"), device=dev)
        acc, count = torch.zeros(2 * (n + 1), dtype=torch.float64, device=dev), torch.zeros(n + 1, dtype=torch.int32, device=dev)
        ws, pd = torch.empty(3 * B, dtype=torch.float64, device=dev), pred.to(dev, dt)
        for _ in range(2):
            L.check(L.lib().vt_sample_metrics(L.ptr(pd), L.dt_code(dt), L.ptr(tgt), L.ptr(mask), L.ptr(sn), L.ptr(rows), B, H, A, n, L.ptr(res),
                                              C.c_void_p(res.data_ptr() + 8 * B), L.ptr(acc), L.ptr(count), L.ptr(ws), L.stream_ptr(torch.device(dev))),
                    "vt_sample_metrics")
        out[f"sample_metrics.{tag}.out"], out[f"sample_metrics.{tag}.acc"], out[f"sample_metrics.{tag}.count"] = res, acc, count
    return out


class _Column:
    """One column of a multi-tensor table: per tensor [pre sentinel words | n values | GUARD sentinel words] on the device, the layout of
    tests/test_gpu_rdt_accum.py; pre = 4 leaves every tensor 16-byte aligned, pre = 5 none."""

    def __init__(self, values, pre, dev):
        self.bufs = [torch.cat([torch.full((pre,), SENTINEL), v.float(), torch.full((GUARD,), SENTINEL)]).to(dev) for v in values]
        self.ptrs = [b.data_ptr() + 4 * pre for b in self.bufs]
        assert all((p % 16 == 0) == (pre % 4 == 0) for p in self.ptrs)

    def whole(self) -> torch.Tensor:
        """every buffer, guard words included, as one tensor: what a digest is taken of"""
        return torch.cat(self.bufs)


def _mt_table(p, g, m, v, sh, dev, no_shadow=()):
    rows, chunk0 = [], 0
    for i, n in enumerate(MT_SIZES):
        rows.append([p.ptrs[i], g.ptrs[i], m.ptrs[i], v.ptrs[i], 0 if i in no_shadow else sh.ptrs[i], n, chunk0])
        chunk0 += (n + 4095) // 4096
    return torch.tensor(rows, dtype=torch.int64).to(dev), chunk0


def _multi_tensor(dev, pre) -> "OrderedDict[str, torch.Tensor]":
    from vlatouch import _lib as L
    from vlatouch.rdt_train import inv_scale
    lib, sp, nt = L.lib(), L.stream_ptr(torch.device(dev)), len(MT_SIZES)
    gen = torch.Generator().manual_seed(2200 + pre)
    draw = lambda: [torch.randn(n, generator=gen) for n in MT_SIZES]
    col = lambda values: _Column(values, pre, dev)
    nans = lambda: [torch.full((n,), float("nan")) for n in MT_SIZES]
    out, tag = OrderedDict(), f"mt.pre{pre}"
    p_h, m_h, v_h, sh_h, g1_h, g2_h, grad_h = draw(), draw(), draw(), draw(), draw(), draw(), draw()
    p, m, v, sh = col(p_h), col(m_h), col(v_h), col(sh_h)
    others = lambda: torch.cat([p.whole(), m.whole(), v.whole()])
    fresh1, fresh2 = col(g1_h), col(g2_h)
    f1, f2 = (torch.tensor(f.ptrs, dtype=torch.int64).to(dev) for f in (fresh1, fresh2))

    # vt_grad_accum_multi: store into NaN-filled accumulators, then add, at scale 1/3
    acc = col(nans())
    tab, chunks = _mt_table(p, acc, m, v, sh, dev)
    L.check(lib.vt_grad_accum_multi(L.ptr(tab), L.ptr(f1), nt, chunks, 1.0 / 3.0, 0, sp), "vt_grad_accum_multi")
    out[f"{tag}.accum.store"] = acc.whole()
    L.check(lib.vt_grad_accum_multi(L.ptr(tab), L.ptr(f2), nt, chunks, 1.0 / 3.0, 1, sp), "vt_grad_accum_multi")
    out[f"{tag}.accum.add"] = acc.whole()
    # vt_grad_fold_pack_multi into a NaN-prefilled exchange buffer (the padding must come out zero), store and add; the accumulators are only read
    comm = None
    for mode, f in (("store", f1), ("add", f2)):
        comm = torch.full((chunks * 4096,), float("nan"), dtype=BF, device=dev)
        L.check(lib.vt_grad_fold_pack_multi(L.ptr(tab), L.ptr(f), nt, chunks, 1.0 / 3.0, int(mode == "add"), L.ptr(comm), sp), "vt_grad_fold_pack_multi")
        out[f"{tag}.fold_pack.{mode}.comm"] = comm
    out[f"{tag}.fold_pack.acc"] = acc.whole()
    out[f"{tag}.fresh"] = torch.cat([fresh1.whole(), fresh2.whole()])
    # vt_grad_unpack_multi: the exchange buffer widened into NaN-filled accumulators
    acc2 = col(nans())
    tab2, _ = _mt_table(p, acc2, m, v, sh, dev)
    L.check(lib.vt_grad_unpack_multi(L.ptr(tab2), L.ptr(comm), nt, chunks, sp), "vt_grad_unpack_multi")
    out[f"{tag}.unpack"] = acc2.whole()
    # vt_ema_multi, the 4097-element row without a shadow
    host = torch.zeros(4)
    L.check(lib.vt_train_hyper(1e-3, 0.9, 0.999, 3, 0.75, L.ptr(host)), "vt_train_hyper")
    tab3, _ = _mt_table(p, acc, m, v, sh, dev, no_shadow=(4,))
    L.check(lib.vt_ema_multi(L.ptr(tab3), nt, chunks, L.ptr(host.to(dev)), sp), "vt_ema_multi")
    out[f"{tag}.ema.shadow"] = sh.whole()
    # vt_grad_clip_multi: clipping (the norm is near 150) and idle
    for mode, max_norm in (("clipping", 1.0), ("idle", 1e9)):
        g = col(grad_h)
        tabc, _ = _mt_table(p, g, m, v, sh, dev)
        part, pair = torch.full((chunks,), float("nan"), device=dev), torch.full((2,), float("nan"), device=dev)
        L.check(lib.vt_grad_clip_multi(L.ptr(tabc), nt, chunks, max_norm, L.ptr(part), L.ptr(pair), sp), "vt_grad_clip_multi")
        out[f"{tag}.clip.{mode}.g"], out[f"{tag}.clip.{mode}.norm_coef"] = g.whole(), pair
    # vt_grad_unscale_clip_multi at S = 3000: finite, and with an inf as the last tensor's last element (nothing may be written then)
    for mode in ("finite", "inf"):
        vals = [x.clone() * 3000.0 for x in grad_h]
        if mode == "inf":
            vals[-1][-1] = float("inf")
        g = col(vals)
        tabu, _ = _mt_table(p, g, m, v, sh, dev)
        part, res = torch.full((chunks,), float("nan"), device=dev), torch.full((4,), float("nan"), device=dev)      # norm, coefficient, flag, one word behind
        L.check(lib.vt_grad_unscale_clip_multi(L.ptr(tabu), nt, chunks, 1.0, inv_scale(3000.0), L.ptr(part), L.ptr(res), C.c_void_p(res.data_ptr() + 8), sp),
                "vt_grad_unscale_clip_multi")
        out[f"{tag}.unscale_clip.{mode}.g"], out[f"{tag}.unscale_clip.{mode}.out"] = g.whole(), res
    out[f"{tag}.p_m_v"] = others()                               # no kernel above writes these
    return out


def parent_cases(dev) -> "OrderedDict[str, str]":
    """name -> sha256 of the output's bytes over the second set."""
    parts = [("fp32.", _elementwise(dev, F32)), ("fp16.", _elementwise(dev, H16)), ("", _elementwise_direct(dev)),
             ("fp32.", _attention(dev, F32, only={("67x20", "wave")})), ("fp16.", _attention(dev, H16, only={("67x20", "wave"), ("67x20", "mfma"), ("128x257", "mfma")})),
             ("", _sample_metrics(dev)), ("", _multi_tensor(dev, 4)), ("", _multi_tensor(dev, 5))]
    out = OrderedDict()
    for prefix, part in parts:
        torch.cuda.synchronize()
        for k, t in part.items():
            out[prefix + k] = digest(t)
    return out

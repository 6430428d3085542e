"""Two saved bf16 cases of the RDT training kernels that gained an fp16 instantiation (csrc/vt_train_rdt.hip, csrc/vt_attn_bwd.hip): seeded
inputs, the calls, and one sha256 digest per output.  tests/golden/g20_bf16_train_kernels.json holds the digests a build of the commit BEFORE
the fp16 mode gave on an MI355X (tools/make_golden_bf16_train.py wrote it, run against that commit's library); the fp16 kernel test recomputes
them, so templating the kernels on the 16-bit type is shown to have left every bf16 bit where it was.  Only calls that commit already had."""
import hashlib
from collections import OrderedDict

import torch

BF = torch.bfloat16
GOLDEN_NAME = "g20_bf16_train_kernels.json"


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _elementwise(dev) -> "OrderedDict[str, torch.Tensor]":
    from vlatouch import _lib as L
    from vlatouch import rdt_train as RT
    g = torch.Generator().manual_seed(20)
    r = lambda *shape: torch.randn(*shape, generator=g)
    out = OrderedDict()
    x, w, dy = (r(5, 256) * 1.7 + 0.3).to(dev, BF), (1 + 0.2 * r(256)).to(dev), r(5, 256).to(dev, BF)
    out["rmsnorm.dx"], out["rmsnorm.dw"] = RT.rmsnorm_bwd(x, w, dy, 1e-6, L.NORM_RMS_MEANSQ)
    out["rmsnorm_var.dx"], out["rmsnorm_var.dw"] = RT.rmsnorm_bwd(x, w, dy, 1e-6, L.NORM_RMS_VAR)
    buf, hw, dbuf = (r(33, 768) * 1.3 + 0.2).to(dev, BF), (1 + 0.2 * r(64)).to(dev), r(33, 768).to(dev, BF)
    out["headnorm.dw"] = RT.headnorm_bwd_(buf[:, 256:512], dbuf[:, 256:512], 4, hw, 1e-6, L.NORM_RMS_VAR)      # 132 pairs: a ragged last group of 64
    out["headnorm.dx"] = dbuf
    a = (r(1000) * 3).to(dev, BF)
    out["gelu"], out["gelu.d"] = RT.act(a, L.ACT_GELU_TANH), RT.act(a, L.ACT_GELU_TANH, r(1000).to(dev, BF))
    out["silu"], out["silu.d"] = RT.act(a, L.ACT_SILU), RT.act(a, L.ACT_SILU, r(1000).to(dev, BF))
    state, action, noise, mask = r(3, 1, 16).to(dev), r(3, 8, 16).to(dev), r(3, 8, 16).to(dev), (r(3, 1, 16) > 0).float().to(dev)
    ts = torch.tensor([3, 437, 998]).to(dev)
    out["qsample"] = RT.ddpm_qsample(state, action, noise, mask, ts, RT.alphas_cumprod(1000, "squaredcos_cap_v2").to(dev), BF)
    out["timestep_embed"] = RT.timestep_embed(ts.float(), RT.timestep_freqs(256).to(dev), BF)
    m = r(33, 40).to(dev, BF)
    pos = r(40).to(dev)
    av = m.clone()
    RT.add_rowvec_(av, pos)
    out["add_rowvec"] = av
    out["transpose_pad"], out["colsum"] = RT.transpose_pad(m), RT.colsum(m)
    out["add"] = RT.add_(m.clone(), r(33, 40).to(dev, BF))
    d = torch.zeros(33, 64, dtype=BF, device=dev)
    RT.copy_cols(m, 7, d, 13, 23)
    out["copy_cols"] = d
    out["mse.loss"], out["mse.dpred"] = RT.mse_loss(m, r(33, 40).to(dev))
    return out


def _attention(dev) -> "OrderedDict[str, torch.Tensor]":
    from vlatouch.rdt_train import attention_bwd
    out = OrderedDict()
    for tag, (B, Nq, Nk, H, masked) in (("67x20", (2, 67, 20, 4, True)), ("128x257", (2, 128, 257, 3, False))):
        g = torch.Generator().manual_seed(Nk)
        qb, kvb = torch.randn(B, Nq, H * 64, generator=g).to(dev, BF), torch.randn(B, Nk, 2 * H * 64, generator=g).to(dev, BF)
        do = torch.randn(B, Nq, H, 64, generator=g).to(dev, BF)
        km = None
        if masked:
            mask = torch.ones(B, Nk, dtype=torch.bool)
            mask[0, Nk - 3:] = False
            mask[1, :] = False
            km = mask.to(dev).to(torch.uint8).contiguous()
        q, k, v = qb.view(B, Nq, H, 64), kvb.view(B, Nk, 2, H, 64)[:, :, 0], kvb.view(B, Nk, 2, H, 64)[:, :, 1]
        for kernel in ("wave", "mfma"):
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

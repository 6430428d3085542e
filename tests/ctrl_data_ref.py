"""Reference statements for the controller store tests: synthetic episodes in the reference's key names, and the batch the two trainers'
`_prepare_batch*` functions build, restated from `make_sample` + `normalize_actions` + `concat_obs` with the CLS rows picked by the
whole-number decision rule (`vlatouch.ctrl_data.norm_decision`)."""
import numpy as np
import torch

from residual_controller.controller_dataset import normalize_actions
from vlatouch import _lib as L
from vlatouch import ctrl_data as CD
from vlatouch import eval as ev
from vlatouch.engine import concat_obs

BRIGHT, DARK = 200, 40      # a frame at 200/255 and one at 40/255: 3 + 1 average 0.63, 1 + 3 average 0.31


def synth_episode(n: int, seed: int, hv: int = 20, fd: int = 3) -> dict:
    """Poses that move from the first frame on, a gripper in counts (0 .. 255), raw VLA chunks and forces."""
    g = np.random.default_rng(seed)
    ee = np.concatenate([np.cumsum(g.normal(scale=0.05, size=(n, 3)), axis=0), g.normal(size=(n, 4))], axis=1)
    vla = g.normal(size=(n, hv, 10))
    vla[:, :, -1] = g.uniform(0, 255, size=(n, hv))
    return {"ee_poses": ee, "gripper_pos": g.uniform(0, 255, size=n), "vla_action": vla, "gelsight_force/forces": g.normal(size=(n, fd))}


def batch_reference(eps, plan, feat, pix, ep_off, P, stats, *, cf, h, layout, use_force, kin, device):
    """eps: episode dicts; plan: [(episode, start)]; feat: fp32 [2][rows][2][dv] and pix: int [2][rows] (host arrays).  -> the mapping
    `ControllerStore.assemble` returns, on the device, and the two decisions."""
    dev = torch.device(device)
    batch = ev.collate([ev.make_sample(eps[e], s, cf, h, use_images=False) for e, s in plan])
    rows = np.array([ep_off[e] + s + cf - 1 for e, s in plan])
    flags = [CD.norm_decision(pix[c][rows], P) for c in range(2)]
    f = [torch.from_numpy(np.ascontiguousarray(feat[c][rows, int(flags[c])])).to(dev) for c in range(2)]
    states, forces = batch["states"], batch["forces"]
    tstats = {k: torch.as_tensor(v, dtype=torch.float32).to(dev) for k, v in stats.items()}
    bridge = layout == "bridge"
    obs = concat_obs(f[0], f[1], states[:, cf - 1], forces[:, cf - 1] if (bridge and use_force) else None, kin, L.F32, dev)
    out = {"obs_in": obs, "expert_act": normalize_actions(batch["expert_actions"], tstats, "expert").to(dev),
           "vla_act": normalize_actions(batch["vla_actions"], tstats, "vla").to(dev)}
    if bridge:
        out["forces"], out["current_force"] = forces[:, cf:].contiguous().to(dev), forces[:, cf - 1].contiguous().to(dev)
    else:
        out["forces"] = forces[:, cf - 1:-1].contiguous().to(dev)
    out["norm_flags"] = torch.tensor([float(flags[0]), float(flags[1])], dtype=torch.float32, device=dev)
    return out

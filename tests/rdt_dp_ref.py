"""Host statements of data-parallel RDT fine-tuning (vlatouch/rdt_train.py with `process_group=`), in plain torch on the CPU.

The bf16 exchange of two ranks: every rank rounds its scaled gradient to bf16 (round to nearest even), the all-reduce adds the two bf16 values
and rounds the sum to bf16 once more: bf16(bf16(a) + bf16(b)).  The sum of two bf16 values (8 significant bits each) is formed here in fp64,
where it is exact up to a span of 45 binades and otherwise equals the larger operand's neighbourhood far from any bf16 tie, and is then
rounded through fp32 to bf16: through fp32 is harmless, because within 16 binades the sum has at most 24 significant bits, and beyond that the
smaller operand is under 2^-16 of the larger, a hundred times closer than the nearest bf16 rounding boundary (2^-9).  The statement is for two
ranks; the order in which a collective adds more than two is its own.

`plan_fields` flattens a SamplePlan into plain values so that two plan streams can be compared field by field."""
import torch


def bf16_rne(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16, round to nearest even (torch's conversion on the CPU; every NaN becomes 0x7FC0)."""
    return x.to(torch.float32).to(torch.bfloat16)


def bf16_exchange(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """bf16(bf16(a) + bf16(b)) for the fp32 tensors a, b of the two ranks -> bf16."""
    return (bf16_rne(a).double() + bf16_rne(b).double()).to(torch.float32).to(torch.bfloat16)


def mixed_values(n: int, seed: int) -> torch.Tensor:
    """n fp32 values of mixed sign and magnitude (1e-6 .. 1e6, a tenth of them zero) with exact bf16 ties (1 + 2^-8 and its like, scaled by
    powers of two) sprinkled in."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * 10.0 ** torch.randint(-6, 7, (n,), generator=g).float() * (torch.rand(n, generator=g) > 0.1)
    ties = (1.0 + 2.0 ** -8 * torch.randint(1, 256, (n,), generator=g).float()) * 2.0 ** torch.randint(-20, 20, (n,), generator=g).float()
    ties = ties * (1 - 2 * torch.randint(0, 2, (n,), generator=g).float())
    return torch.where(torch.rand(n, generator=g) < 0.2, ties, x)


def plan_fields(p) -> tuple:
    """Every field of a vlatouch.rdt_data.SamplePlan as plain, comparable values."""
    jit = tuple(None if j is None else (tuple(j.order), tuple(j.factors())) for j in p.jitter)
    return (p.episode, p.step_id, p.action_id, p.ctrl_masked, p.state_masked, p.elem_masked, tuple(p.frame_idx), tuple(p.slot_valid),
            tuple(p.frame_valid), None if p.noise is None else tuple(float(v) for v in p.noise), p.noise_snr, jit)

"""Periodic sampling evaluation — mirror of the reference's VLA/train/sample.py:7-98 (`log_sample_res`).

Same signature and the same returned dict; the work is vlatouch.rdt_train.sample_eval: `rdt.predict_action` on the device, one
vt_sample_metrics launch per batch, one device read at the end.  Differences from the reference: `weight_dtype` is not applied to the batch
(the runner casts its inputs to its own dtype, and the error is formed in fp32 from the returned prediction where the reference forms
F.mse_loss in weight_dtype before `.float()`); a batch may carry ready `img_tokens` instead of `images`, and an `x_init`; `accelerator`
is None (one process) or any object with a `process_group` attribute: with a group every rank evaluates its own `num_sample_batches` batches,
the sums are all-reduced once and the overall pair is divided by num_sample_batches times the world size, the reference's
`accelerator.gather(...).mean()` (sample.py:80-85)."""
from __future__ import annotations

from vlatouch.rdt_train import sample_eval


def log_sample_res(text_encoder, vision_encoder, rdt, args, accelerator, weight_dtype, dataset_id2name, dataloader, logger):
    if logger is not None:
        logger.info(f"Running sampling for {args.num_sample_batches} batches...")
    return sample_eval(rdt, dataloader, num_sample_batches=args.num_sample_batches, dataset_id2name=dataset_id2name,
                       vision_encoder=vision_encoder, text_encoder=text_encoder, group=getattr(accelerator, "process_group", None))

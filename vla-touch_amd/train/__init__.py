"""Mirror of the reference's VLA/train package: the pieces of its fine-tuning run that exist here (sample.py)."""

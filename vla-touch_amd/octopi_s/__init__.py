"""Mirror of the reference's octopi/octopi_s package: the planning-level tactile encoder (utils/encoder.py)."""

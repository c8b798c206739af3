"""Model-based NPG (reference mjrl/algos/model_accel/): learned dynamics ensembles fitted, rolled out and checked for
disagreement on the GPU through libmjx (csrc/dynamics.h)."""

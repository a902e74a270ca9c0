"""Drop-in `metrics` package (reference metrics/): the FID leg and R-precision on the HIP kernels."""
from .r_precision import r_precision_hits, r_precision_mean_std  # noqa: F401

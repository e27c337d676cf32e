"""rho_diffusion.metrics (the reference's package; ``losses`` is built here, ``geom`` - WassersteinWrapper, which needs
geomloss - is not)."""
from . import losses
from .losses import approx_standard_normal_cdf, discretized_gaussian_log_likelihood, normal_kl

__all__ = ["losses", "normal_kl", "approx_standard_normal_cdf", "discretized_gaussian_log_likelihood"]

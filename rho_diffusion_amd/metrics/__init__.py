"""rho_diffusion.metrics (the reference's package): ``losses`` (guided-diffusion's VLB terms) and ``geom`` (WassersteinWrapper: the
Sinkhorn divergence of geomloss, restated here and run as HIP kernels), plus ``PeakSignalNoiseRatio``, the metric the reference's
pipelines take from torchmetrics, and ``StructuralSimilarityIndexMeasure`` of the same package (one fused HIP kernel, 1 to 3 spatial
dimensions)."""
from . import geom, losses, psnr, ssim
from .geom import SinkhornDivergence, WassersteinWrapper, epsilon_schedule
from .losses import approx_standard_normal_cdf, discretized_gaussian_log_likelihood, normal_kl
from .psnr import PeakSignalNoiseRatio
from .ssim import StructuralSimilarityIndexMeasure

__all__ = ["losses", "geom", "psnr", "ssim", "normal_kl", "approx_standard_normal_cdf", "discretized_gaussian_log_likelihood",
           "SinkhornDivergence", "WassersteinWrapper", "epsilon_schedule", "PeakSignalNoiseRatio",
           "StructuralSimilarityIndexMeasure"]

"""Datasets of the reference (rho_diffusion/data/): the synthetic spherical-harmonic fields (``synthetic``), DeepGalaxy images
(``deep_galaxy``), rotational spectra (``spectroscopy``), MNIST / CIFAR-10 from files on disk (``wrappers``) and the discrete parameter spaces their labels live in (``parameter_space``)."""
from .parameter_space import AbstractParameterSpace, DiscreteParameterSpace  # noqa: F401
from .synthetic import (SphericalHarmonicDataset, SphericalHarmonicPool, spherical_harmonic_field,  # noqa: F401
                        spherical_harmonic_fields)
from .deep_galaxy import DeepGalaxyDataset  # noqa: F401
from .spectroscopy import SpectroscopyDataset  # noqa: F401
from .wrappers import CIFAR10Dataset, MNISTDataset  # noqa: F401

__all__ = ["spherical_harmonic_fields", "spherical_harmonic_field", "SphericalHarmonicPool", "SphericalHarmonicDataset",
           "AbstractParameterSpace", "DiscreteParameterSpace", "DeepGalaxyDataset", "SpectroscopyDataset", "MNISTDataset",
           "CIFAR10Dataset"]

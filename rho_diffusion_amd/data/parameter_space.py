"""Parameter spaces of the reference's conditional datasets (rho_diffusion/data/parameter_space.py:19-92): a name -> value-list mapping
with dict access, the number of value combinations (``size``) and random draws from their Cartesian product
(``utils.sample_from_discrete_parameter_space``).  ``MultiEmbeddings(parameter_space=...)`` takes one as it takes a dict
(scripts/training.py:119 passes ``DeepGalaxyDataset.parameter_space``)."""
from __future__ import annotations

import math
from abc import ABC
from collections import OrderedDict
from typing import Any, Union

import numpy as np

from ..utils import sample_from_discrete_parameter_space

__all__ = ["AbstractParameterSpace", "DiscreteParameterSpace", "sample_from_discrete_parameter_space"]


class AbstractParameterSpace(ABC):
    """parameter_space.py:19-65."""

    def __init__(self, param_dict=None, sampler=None):
        self.param_dict = param_dict if param_dict is not None else OrderedDict()
        self.sampler = sampler

    def set(self, param_dict: Union[dict, OrderedDict]) -> None:
        self.param_dict = param_dict

    @property
    def parameters(self):
        return self.param_dict.keys()

    def sample(self, num_samples, device=None):
        raise NotImplementedError("Method sample() is not implemented.")

    def size(self):
        raise NotImplementedError("Method size() is not implemented.")

    def push_parameter(self, key: str, value: Any) -> None:
        raise NotImplementedError("Method push_parameter() is not implemented.")

    def __repr__(self) -> str:
        return self.param_dict.__repr__()

    def __getitem__(self, key) -> Any:
        return self.param_dict[key]

    def __setitem__(self, key, value):
        self.param_dict[key] = value

    def __len__(self) -> int:
        return len(self.param_dict)

    def items(self):
        return self.param_dict.items()

    def values(self):
        return self.param_dict.values()

    def keys(self):
        return self.param_dict.keys()


class DiscreteParameterSpace(AbstractParameterSpace):
    """parameter_space.py:68-92.  ``size()`` is the product of the value-list lengths (the reference counts the enumerated product;
    an empty space fails in both with the same ValueError).  ``push_parameter``: a key holding None becomes [] (as the reference);
    for a key holding values the reference's branch calls ``isinstance`` with one argument and raises TypeError, so here the branch
    does what it spells out: a list / array appends each value not yet present, a scalar is appended when not present."""

    def __init__(self, param_dict=None, sampler=None):
        super().__init__(param_dict=param_dict, sampler=sampler)
        self.sampler = sample_from_discrete_parameter_space if sampler is None else sampler

    def sample(self, num_samples, device=None):
        return self.sampler(self.param_dict, batch_size=num_samples, random=True, device=device)

    def size(self):
        keys, values = zip(*self.param_dict.items())
        return math.prod(len(v) for v in values)

    def push_parameter(self, key: str, value: Any) -> None:
        if self.param_dict[key] is None:
            self.param_dict[key] = []
        elif isinstance(value, (list, np.ndarray)):
            for v in value:
                if v not in self.param_dict[key]:
                    self.param_dict[key].append(v)
        elif value not in self.param_dict[key]:
            self.param_dict[key].append(value)

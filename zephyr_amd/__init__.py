"""zephyr_amd -- MI355X-native frequency-domain Helmholtz forward solver behind Zephyr's
backend operator API (`Disc(systemConfig) * rhs`, `MultiFreq(systemConfig) * rhs`).

Host classes mirror zephyr.backend; all assembly and solves run in libhelm (HIP, gfx950).
"""
from .analytical import AnalyticalHelmholtz
from .base import BaseModelDependent, BaseAnisotropic
from .config import AttributeMapper, BaseSCCache, SCFilter
from .discretization import BaseDiscretization, DiscretizationWrapper, prefactor_many
from .distributors import (BaseDist, BaseMPDist, MultiFreq, SerialMultiFreq, ViscoMultiFreq, MultiGridHelper, MultiGridMultiFreq,
                           ViscoMultiGridMultiFreq)
from .eurus import Eurus, EurusHD
from .helm3d import Helm3D, Helm3DTransposed
from .interpolation import BaseGridInterpolator, SplineGridInterpolator
from .minizephyr import MiniZephyr, MiniZephyrHD, MiniZephyr25D
from .misfit import DataMisfit
from .source import (FakeSource, SimpleSource, StackedSimpleSource, SparseKaiserSource, KaiserSource,
                     AnisotropicKaiserSource)
from .survey import Helm3DSurvey
from .problem3d import Helm3DProblem

def trim():
    'give the scratch memory libhelm caches between calls (tens of GB after large direct solves) back to the device'
    from . import _lib
    return _lib.load().helm_trim()


__all__ = [
    'AnalyticalHelmholtz', 'BaseModelDependent', 'BaseAnisotropic', 'AttributeMapper', 'BaseSCCache', 'SCFilter',
    'BaseDiscretization', 'DiscretizationWrapper', 'prefactor_many', 'BaseDist', 'BaseMPDist', 'MultiFreq', 'SerialMultiFreq',
    'ViscoMultiFreq', 'MultiGridHelper', 'MultiGridMultiFreq', 'ViscoMultiGridMultiFreq', 'BaseGridInterpolator', 'SplineGridInterpolator', 'Eurus', 'EurusHD', 'Helm3D', 'Helm3DTransposed', 'MiniZephyr', 'MiniZephyrHD', 'MiniZephyr25D', 'FakeSource', 'SimpleSource',
    'StackedSimpleSource', 'SparseKaiserSource', 'KaiserSource', 'AnisotropicKaiserSource', 'Helm3DSurvey', 'Helm3DProblem', 'DataMisfit', 'trim',
]

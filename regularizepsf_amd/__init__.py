"""MI355X-native patch-wise Fourier PSF correction with the regularizepsf class API.

Drop-in for the ``ArrayPSFBuilder`` / ``ArrayPSF`` / ``ArrayPSFTransform`` / ``IndexedCube`` / ``calculate_covering`` path (and
the functional PSF models that feed it) of
punch-mission/regularizepsf (regularizepsf/__init__.py:5-16 re-exports the same names); the compute
runs in hand-written HIP kernels behind the C ABI of include/rpsf.h.
"""

from regularizepsf_amd.exceptions import (
    FunctionParameterMismatchError,
    IncorrectShapeError,
    InvalidCoordinateError,
    InvalidDataError,
    InvalidFunctionError,
    PSFBuilderError,
    RegularizePSFError,
)
from regularizepsf_amd.functional import (
    SimpleFunctionalPSF,
    VariedFunctionalPSF,
    elliptical_gaussian,
    moffat,
    simple_functional_psf,
    varied_functional_psf,
)
from regularizepsf_amd._native import pinned_empty
from regularizepsf_amd.builder import ArrayPSFBuilder, build_iterative, build_subtracted, scale_image
from regularizepsf_amd.device_array import DeviceArray, device_empty, to_device
from regularizepsf_amd.psf import ArrayPSF
from regularizepsf_amd.stars import (cell_fit_summary, find_stars, fit_groups, fit_positions, fit_stars, fit_stars_weighted, refine_stars,
                                     render_stars, star_catalog, star_groups, star_photometry, subtract_stars)
from regularizepsf_amd.transform import ArrayPSFTransform
from regularizepsf_amd.util import IndexedCube, calculate_covering

__version__ = "0.1.0"

__all__ = [
    "ArrayPSF",
    "ArrayPSFBuilder",
    "ArrayPSFTransform",
    "DeviceArray",
    "FunctionParameterMismatchError",
    "IncorrectShapeError",
    "IndexedCube",
    "InvalidCoordinateError",
    "InvalidDataError",
    "InvalidFunctionError",
    "PSFBuilderError",
    "RegularizePSFError",
    "SimpleFunctionalPSF",
    "VariedFunctionalPSF",
    "build_iterative",
    "build_subtracted",
    "calculate_covering",
    "cell_fit_summary",
    "device_empty",
    "elliptical_gaussian",
    "find_stars",
    "fit_groups",
    "fit_positions",
    "fit_stars",
    "fit_stars_weighted",
    "moffat",
    "pinned_empty",
    "refine_stars",
    "render_stars",
    "scale_image",
    "simple_functional_psf",
    "star_catalog",
    "star_groups",
    "star_photometry",
    "subtract_stars",
    "to_device",
    "varied_functional_psf",
]

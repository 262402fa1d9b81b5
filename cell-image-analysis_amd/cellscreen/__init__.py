"""cellscreen -- host-side mirror of the reference's screening/training interface over
libcellscreen.so (hand-written gfx950 HIP).  Importing this package loads no native code;
Engine / ProductionMutantScreening do, and fail loudly when the library or a GPU is missing."""
from . import spec  # noqa: F401
from .colocalize import ColocalizationMeasurer, ColocalizationTable, colocalization_table, colocalize_params  # noqa: F401
from .expand import LabelExpander, expand_params  # noqa: F401
from .granularity import GranularityMeasurer, GranularityTable, granularity_params, granularity_table  # noqa: F401
from .illumination import IlluminationCorrector, IlluminationFunction  # noqa: F401
from .intensity import IntensityMeasurer, ObjectTable  # noqa: F401
from .neighbors import NeighborMeasurer, NeighborTable, neighbor_params, neighbor_table  # noqa: F401
from .propagate import LabelPropagator, propagate_params  # noqa: F401
from .quality import ImageQualityMeasurer, ImageQualityTable, ObjectFocusTable, image_quality_table, object_focus_table  # noqa: F401
from .quantile import QuantileMeasurer, QuantileTable  # noqa: F401
from .radial import RadialMeasurer, RadialTable, radial_params, radial_table  # noqa: F401
from .shape import ShapeMeasurer, ShapeTable, shape_table  # noqa: F401
from .spec import CAEWeights, DetectorParams, OCSVMParams  # noqa: F401
from .spots import SpotDetector, SpotTable, dog_noise_gain, spot_params, spot_table  # noqa: F401
from .texture import TextureMeasurer, TextureTable, texture_table  # noqa: F401

__all__ = ["spec", "CAEWeights", "DetectorParams", "OCSVMParams", "LabelExpander", "expand_params", "IntensityMeasurer",
           "ObjectTable", "QuantileMeasurer", "QuantileTable", "TextureMeasurer", "TextureTable", "texture_table",
           "ShapeMeasurer", "ShapeTable", "shape_table", "NeighborMeasurer", "NeighborTable", "neighbor_params", "neighbor_table",
           "ColocalizationMeasurer", "ColocalizationTable", "colocalization_table", "colocalize_params",
           "RadialMeasurer", "RadialTable", "radial_params", "radial_table",
           "GranularityMeasurer", "GranularityTable", "granularity_params", "granularity_table", "LabelPropagator", "propagate_params",
           "ImageQualityMeasurer", "ImageQualityTable", "ObjectFocusTable", "image_quality_table", "object_focus_table",
           "SpotDetector", "SpotTable", "dog_noise_gain", "spot_params", "spot_table", "IlluminationCorrector", "IlluminationFunction"]

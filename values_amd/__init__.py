"""values_amd -- MI355X-native hot path of ValUES' multi-pass segmentation-uncertainty inference."""
from .unet3d import UNet3D  # noqa: F401
from .ssn import SsnUNet3D  # noqa: F401
from .uncertainty import (calculate_one_minus_msr, calculate_uncertainty, one_minus_msr_batch, softmax_variance,  # noqa: F401
                          uncertainty_maps)
from .predict import (GraphedPredictor, HostPipeline, crop_indices, noise_view_device, predict_logits,  # noqa: F401
                      predict_uncertainty)
from .io import load_models_from_checkpoint, instantiate  # noqa: F401
from .sliding import predict_image_sliding, run_test_3d  # noqa: F401
from .preprocess import load_cases_device, preprocess_dataset  # noqa: F401
from .preprocess2d import preprocess_dataset_2d, preprocess_images_device  # noqa: F401
from .toydata import generate_toy_dataset  # noqa: F401
from .stl import generate_toy_dataset_from_config  # noqa: F401
from . import validation  # noqa: F401
from .validation import validate, validate_split, validation_step  # noqa: F401
from . import datamodule3d  # noqa: F401
from .datamodule3d import DeviceLoader3D, HostLoader3D, LIDCDataModule3D, ToyDataModule3D  # noqa: F401

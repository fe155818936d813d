"""The reference keeps its dataset beside the model (audio_models/RCNN_KWS/qualcomm_kws_dataset.py); here it lives in
datasets/qualcomm_kws_dataset.py and is importable from both places."""
from datasets.qualcomm_kws_dataset import *  # noqa: F401,F403
from datasets.qualcomm_kws_dataset import USAGE_SLICES  # noqa: F401

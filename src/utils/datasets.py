"""`from src.utils.datasets import get_dataset`."""
from loopy_slam_amd.datasets import get_dataset, BaseDataset, Replica, ScanNet, Azure, TUM_RGBD, dataset_dict  # noqa: F401

from .kitti_v2 import KittiDepthV2  # noqa: F401
from .waymo import WaymoDepth  # noqa: F401

from .build import DEPTH_NET_REGISTRY, build_depth_net  # noqa: F401
from .DepthResNet import DepthResNet  # noqa: F401
from .PackNet01 import PackNet01  # noqa: F401
from .BTSNet import BtsModel  # noqa: F401
from .GoogleResNet import GoogleResNet  # noqa: F401
from .GoogleResNetv2 import GoogleResNetv2  # noqa: F401

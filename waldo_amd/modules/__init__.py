from .warp import TPSWarp, InverseWarp, kernel_distance  # noqa: F401
from .conv import UNet  # noqa: F401

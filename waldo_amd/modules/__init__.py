from .warp import TPSWarp, InverseWarp, kernel_distance  # noqa: F401
from .conv import UNet, ConvPatchProj  # noqa: F401
from .transform import Block, ClipPlan, MultiBlocks  # noqa: F401

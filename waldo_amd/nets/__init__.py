from .lvd import (Warper, compute_occ, reduce_comp, gather_time, scale,  # noqa: F401
                  estimate_alpha_grid_occ, decode_output, ImageEncoder, ImageDecoder, PoseEstimator,
                  LayerEstimator, LVD, lvd_net_opt, get_circle)
from .wif import WIF  # noqa: F401
from .flp import FLP, FlpPlan, LatentCompressor, PoseDecoder, PoseEncoder, flp_net_opt  # noqa: F401
from .lpips import LPIPS  # noqa: F401

"""MI355X-native FlowDiffuser hot path (gfx950): hand-written HIP kernels behind the reference's
`algorithms.diffusion_animation` plugin surface.  See DESIGN.md / INTEGRATION.md."""
from .warp import warp, nan_mse, nan_mse_rows, scale, warp_forward_flow, warp_backward_flow, interpolate_frames, upsample_flow, loop_frames, integrate_flow  # noqa: F401
from .warp import (flow_consistency, FlowConsistency, STATE_HELD, STATE_RELEASED, STATE_INCONSISTENT, STATE_LEAVES_FRAME,  # noqa: F401
                   STATE_UNMATCHED, STATE_INVALID)
from .warp import median_filter_flow, median_params  # noqa: F401
from .warp import chain_flows, chain_flows_to, composite_layer, FlowChain  # noqa: F401
from .warp import fit_motion, motion_flow, warp_homography, camera_path, stabilize_clip, motion_params, MotionFit  # noqa: F401
from .warp import segment_motion, assign_motion, vote_labels, layers_params, MotionLayers, LABEL_OUTLIER, LABEL_INVALID  # noqa: F401
from .warp import build_plate, project_plate, background_plate, remove_moving, plate_params, plate_canvas, plate_voters, Plate  # noqa: F401
from .warp import temporal_filter, temporal_params, TemporalFilter  # noqa: F401
from .warp import fill_along_tracks, complete_flows, inpaint_clip, clipfill_params, ClipFill  # noqa: F401
from .warp import harmonic_fill, seamless_clone, membrane_params, HarmonicFill, SeamlessClone  # noqa: F401
from .softsplat import softsplat  # noqa: F401
from .denoising_diffusion import Unet, ConditionalDiffusion, PhotoGuide  # noqa: F401,E402
from .flow_diffuser import FlowDiffuser, UnetWithWarp  # noqa: F401,E402
from .flow_learner import FlowLearner  # noqa: F401,E402
from .flow_pred import FlowPred, Autoencoder  # noqa: F401,E402
from .frame_generator import FrameGenerator  # noqa: F401,E402
from .flow_completer import FlowCompleter  # noqa: F401,E402

"""fast_scnn_pytorch_amd — MI355X-native (gfx950) Fast-SCNN forward/backward hot path.

Importable as ``fast_scnn_pytorch_amd`` via ``_fscnn_boot.load()`` (the directory name has a
hyphen).  The drop-in module for reference callers is the top-level ``models`` package.

Submodules:
  arch           canonical tensor table (state_dict schema of models/fast_scnn.py)
  portable_init  counter-based weight / input generator (no torch RNG)
  _lib           ctypes binding of the C-ABI library libfastscnn_hip.so (fails loudly if absent)
  fast_scnn      FastSCNN / get_fast_scnn — the reference interface, running on HIP kernels
  loss           fused cross-entropy criterion (HIP)
  optim          fused multi-tensor SGD and AdamW (HIP)
  ddp            one-process-per-GPU data parallel with bucketed RCCL gradient all-reduce
  deploy         EndToEndFastSCNN — the deployment model: raw frames in, probabilities / mask out
  bev            BirdEyeView / centerline / warp_image — calibration, view parameters, the
                 centreline read from the row table of EndToEndFastSCNN.bird_eye, and the colour
                 bird's-eye view of a camera frame (EndToEndFastSCNN.bird_eye_view)
  path           plan / PathPlanner / VisualLateralErrorController — the steering tail: row table
                 -> fitted path -> wheel PWM in one launch (EndToEndFastSCNN.steer runs it behind
                 the bird's-eye tail)
  vis            overlay_mask — the lane / class overlay of a frame and a mask on the device
                 (EndToEndFastSCNN.overlay is the same blend fused behind the backbone)
"""
__all__ = ["FastSCNN", "get_fast_scnn", "EndToEndFastSCNN", "BirdEyeView", "centerline",
           "overlay_mask", "warp_image"]


def __getattr__(name):
    if name in ("FastSCNN", "get_fast_scnn"):
        from . import fast_scnn
        return getattr(fast_scnn, name)
    if name == "EndToEndFastSCNN":
        from . import deploy
        return deploy.EndToEndFastSCNN
    if name in ("BirdEyeView", "centerline", "warp_image"):
        from . import bev
        return getattr(bev, name)
    if name == "overlay_mask":
        from . import vis
        return vis.overlay_mask
    raise AttributeError(name)

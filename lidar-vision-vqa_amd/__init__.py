"""lidar-vision-vqa_amd -- MI355X-native LiDAR+vision fusion hot path.

Import name: `lidar_vision_vqa_amd` (the root-level shim `lidar_vision_vqa_amd.py` maps it onto this
directory, whose on-disk name carries a hyphen).  Sub-packages:

  lidar   voxeliser / VFE / BEV-scatter plugins with the OpenPCDet `batch_dict` protocol
  dense_head  CenterHead (BEV features -> 3-D boxes: conv stack, top-K decode, rotated BEV NMS) with the reference's module API
  sparse_head VoxelNeXtHead (the sparse BEV rows of VoxelResBackBone8xVoxelNeXt -> 3-D boxes: fused branch convs, top-K over rows) and the
              registry of both heads, dense_heads_all
  anchor_head AnchorHeadSingle (BEV features -> a box for every anchor: one fused 1 x 1 conv, anchor decode) and post_processing (score mask,
              top 4096, rotated BEV NMS over 64 mask words), the detectors' class-agnostic route; dense_heads_all with all three heads
  transfusion_head TransFusionHead (BEV features -> heat-map proposals -> one decoder layer over the H W key stream -> 3-D boxes: proposals,
              query gather, learned position embeddings, fused FFN + branches + decode) ; dense_heads_all with all four heads
  fusion  VATBlock / VATLiDAR / VATVision / VisionAdapter with the reference's nn.Module API
  vision_tower  the SAM ViT image encoder (ImageEncoderViT, build_sam_vit_b) with the reference's nn.Module API
  head    prefix assembly + stand-in decoder head
  dist    scene sharding + fused all-reduce over RCCL
  _ffi    ctypes binding of the C-ABI library built from csrc/ (include/lvq.h)
  synth   synthetic scenes / weights (no dataset or checkpoint is reachable offline)
"""
__version__ = "0.1.0"

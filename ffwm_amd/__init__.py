"""ffwm_amd -- MI355X (gfx950) implementation of the flow-guided feature-warping hot path of
csyxwei/FFWM: hand-written HIP kernels behind the reference's own operator API.

    ffwm_amd.external_function   BlockExtractor / LocalAttnReshape / Resample2d (+Function.apply),
                                 WarpNet, WarpFlipCat, IdentityInputFunction (the identity network's input, --crop included)
    ffwm_amd.losses              the reference's callers restated: AffineRegularizationLoss, PerceptualCorrectness,
                                 IdentityLoss(lightcnn, crop) -- trainer.FFWMTrainer(..., crop=True) trains against the cropped face;
                                 MultiScaleLDLoss / LandmarkLoss(fused=True): all scales and their flow gradients in one call;
                                 ClassifierLoss(fused=True): cross entropy over 79 077 classes, its gradient, prec@1 / prec@5 in one call
    ffwm_amd.trainer             FFWMTrainer (train_ffwm.py; load_pretrained_flow takes --flownetf / --flownetb, load_lightcnn
                                 --lightcnn), FlowNetTrainer (train_flow.py, reverse=True is --reverse; save_networks writes
                                 <epoch>_net_flowNet.pth) and LightCNNTrainer (lightcnn/finetune.py: the reference's parameter groups,
                                 learning-rate schedule, validation and lightCNN_<n>_checkpoint.pth files)
    ffwm_amd.optim               FlatAdam and FlatSGD: an optimizer step as one streaming kernel over the reducer's flat arrays
    ffwm_amd.compat              block_extractor_cuda / local_attn_reshape_cuda / resample2d_cuda shims
    ffwm_amd.ops                 tensor-level calls into the C ABI (include/ffwm_hip.h)
    ffwm_amd.build               hipcc build recipe for ffwm_amd/lib/libffwm_hip.so
    ffwm_amd.Frontalizer         inference as the reference's test_ffwm.py runs it: flowNetF -> WarpNet -> netG from two
                                 checkpoints, one captured hipGraph (ffwm_amd.ffwm_eval; FoldedFFWM is the generator alone)
    ffwm_amd.FaceIdentifier      the rest of that loop: Frontalizer -> (centre-face crop) -> LightCNN-29 feature -> cosine top-k
                                 against a gallery, one captured hipGraph (ffwm_amd.identity_eval; FoldedLightCNN is the feature
                                 network alone, IdentityResult what a call returns, RankMeter the by-pose rank-1 meter)
    ffwm_amd.FaceStore           the reference's FaceDataset with --preload, kept on the device as bytes (ffwm_amd.data: from_directory /
                                 from_arrays / .npz, pairs, s2f, the gallery, host_item / host_batch as the CPU path), and
    ffwm_amd.FaceLoader          its DataLoader: one uploaded permutation per epoch, one gather launch per batch (csrc/face_batch.hip),
                                 batches in the form the trainers' step() and capture() take; rotation=True on both is the random
                                 rotation of --aug as a stated algorithm (cv2.warpAffine's fixed-point path; no OpenCV confirmed it)
    ffwm_amd.IdentityStore       the reference's lightcnn ImgDataset with --preload on the device (bytes and classes), and
    ffwm_amd.IdentityLoader      its DataLoader: PIL's bicubic RandomRotation(5), the flip, the channel mean and --crop of a whole batch
                                 in one launch (csrc/identity_batch.hip); LightCNNTrainer.train_epoch(loader, epoch) runs an epoch
    ffwm_amd.ResultWriter        the reference's result images (util/util.py tensor2im / tensor2mask / tensor2flow / tensor2att,
                                 flow_util.flow2img, the Visualizer's routing and file names): a whole batch of visuals as uint8 RGB
                                 sheets from one call (csrc/visuals.hip), one copy to the host, PNGs through PIL (ffwm_amd.visuals:
                                 render, from_result, train_visuals, and the numpy restatements that are the CPU path)
"""
__version__ = "0.1.0"


def __getattr__(name):
    # imported on first use: `import ffwm_amd` stays free of torch
    if name in ("Frontalizer", "FoldedFFWM", "FrontalizerResult"):
        from . import ffwm_eval
        return getattr(ffwm_eval, name)
    if name in ("FaceIdentifier", "FoldedLightCNN", "IdentityResult", "RankMeter"):
        from . import identity_eval
        return getattr(identity_eval, name)
    if name in ("FaceStore", "FaceLoader", "FaceBatch", "IdentityStore", "IdentityLoader", "IdentityBatch"):
        from . import data
        return getattr(data, name)
    if name == "ResultWriter":
        from . import visuals
        return visuals.ResultWriter
    raise AttributeError("module %r has no attribute %r" % (__name__, name))

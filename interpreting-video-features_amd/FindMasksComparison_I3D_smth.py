"""Drop-in for video_features_pytorch/FindMasksComparison_I3D_smth.py on the MI355X.

    python FindMasksComparison_I3D_smth.py -c configs/config_i3d_smth.py --msl "" \
        --checkpoint ckpt.pth.tar --subDir run0 [--synthetic 16]

`find_masks` keeps the reference's positional signature (smth:125-126).
"""
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ivf_find_masks  # noqa: E402
import utils  # noqa: E402

RESIZE_SIZE_WIDTH = 224
RESIZE_SIZE_HEIGHT = 224
_state = {"sub_dir": "run0"}


def find_masks(dat_loader, model, hyper_params, lam1, lam2, N, maskType="gradient", temporalMaskType="freeze",
               classOI=None, verbose=True, maxMaskLength=None, doGradCam=False, runTempMask=True, maskGrid=None,
               maskSigma=None, lam3=None, maxBox=None, doIntGrad=False, igSteps=32, igBaseline="frozen", doRise=False,
               riseMasks=1024, riseProb=0.5, riseGrid=None, riseSigma=None, riseSeed=0, doSmoothGrad=False, sgSamples=32,
               sgLevel=0.15, sgSeed=0, doShapley=False, shapPerms=64, shapGrid=None, shapSigma=None, shapSeed=0,
               doCurves=False, curveGrid=None, curveSigma=None, curveStep=1, camKinds=(), camTarget=None,
               doScoreCam=False, scoreCamTarget=None, scoreCamWeights="increase", scoreCamPerturb="freeze",
               scoreCamSigma=None, scoreCamChannels=None, doKernelShap=False, kshapSamples=256, kshapGrid=None,
               kshapSigma=None, kshapSeed=0, doLime=False, limeSamples=1024, limeProb=0.5, limeGrid=None, limeSigma=None,
               limeSeed=0, limeWidth=0.25, limeRidge=1.0):
    """smth:125-315.  doKernelShap and doLime (extensions; whatever the maskType; freeze only) also fit a linear
    surrogate of the score drop in the frozen cells of kshapGrid / limeGrid (gt, gh, gw) (default (T, 1, 1): the frames),
    blurred by kshapSigma / limeSigma input pixels, forward passes only, the least-squares fit in fp64 on the device --
    KernelSHAP on kshapSamples paired coalitions with Shapley-kernel sizes drawn from kshapSeed (the values sum to the
    score drop of the fully frozen clip), LIME on limeSamples rows that freeze a cell with probability limeProb, drawn from
    limeSeed, weighted by an exponential kernel of width limeWidth, with ridge limeRidge and a free intercept -- and write
    further pickles (KernelShap, Lime in place of GradCam) of records with 'KshapHeatMap' [T,H,W], 'KshapCells'
    [gt,gh,gw], 'KshapFrames' [T], 'kshap_total', 'kshap_ok', 'kshap_r2', 'n_samples', 'seed', and 'LimeHeatMap',
    'LimeCells', 'LimeFrames', 'lime_intercept', 'lime_ok', 'lime_r2', 'n_samples', 'seed'; doCurves ranks the maps under
    'kshap' and 'lime'.  doScoreCam (an extension; whatever the maskType) also runs Score-CAM on scoreCamTarget
    (default: the Grad-CAM target; scoreCamChannels = (first, count) a window of its channels) -- a forward pass per
    channel with the channel's normalised map as the mask, blurred by scoreCamSigma input pixels, applied as
    scoreCamPerturb 'freeze' or 'blank', weighted as scoreCamWeights 'increase' or 'softmax' -- and writes a further
    pickle (ScoreCam in place of GradCam) of records with 'ScoreCamHeatMap', 'ScoreCamWeights', 'ScoreCamValid',
    'score_base', 'layer', 'weights', 'perturb'; doCurves ranks it under 'scorecam'.  maskType 'combi' runs the exhaustive one-blob search over masks of length <= maxMaskLength
    (smth:137-141, no gradient descent; N is unused); any other maskType keeps the gradient search from
    init_mask(mode="central"), which the reference hard-codes (smth:190).  maskType 'spacetime' (an extension, no
    counterpart in the reference) searches a mask per frame and cell of a maskGrid (gh, gw) grid, blurred by maskSigma
    input pixels, with lam3 on the spatial TV term; records also carry 'st_mask' [T,gh,gw].  maskType 'stcombi' (an
    extension as well) is the exhaustive counterpart of 'spacetime': every box of one temporal blob (length <=
    maxMaskLength, default T) times one rectangle of at most maxBox = (mh, mw) grid cells (default the whole grid) is
    scored and the minimiser of the spacetime loss kept; N is unused; records also carry 'st_mask' (binary),
    'box_start', 'box_length', 'box_rows', 'box_cols' and 'box_drop'.  doIntGrad (an extension as well, whatever the
    maskType) also runs Integrated Gradients with igSteps midpoint nodes from the igBaseline ('frozen' or 'constant')
    and writes a third pickle of records with 'IGHeatMap' [T,H,W], 'IGFrames' [T], 'ig_total', 'ig_gap', 'score_base'.
    doRise (an extension as well, whatever the maskType; freeze only) also runs RISE random-mask saliency -- riseMasks
    random masks on riseGrid (gt, gh, gw), each cell frozen with probability riseProb, blurred by riseSigma input pixels,
    drawn from riseSeed, forward passes only -- and writes a further pickle of records with 'RiseHeatMap' [T,H,W],
    'RiseCells' and 'RiseCount' [gt,gh,gw], 'RiseFrames' [T], 'rise_mean_drop', 'n_masks', 'p', 'seed'.
    doSmoothGrad (an extension as well, whatever the maskType) also runs SmoothGrad, SmoothGrad^2 and VarGrad -- sgSamples
    noisy copies of the clip, noise of standard deviation sgLevel * (max - min) of the clip drawn from sgSeed, one forward
    and backward each -- and writes a further pickle of records with 'SGHeatMap', 'SGSqHeatMap', 'SGVarHeatMap' [T,H,W],
    'SGFrames' [T], 'sigma', 'n_samples', 'level', 'seed'.
    doShapley (an extension as well, whatever the maskType; freeze only) also runs Shapley value sampling -- shapPerms
    permutations of the cells of shapGrid (gt, gh, gw) (default (T, 1, 1): the frames are the players), blurred by
    shapSigma input pixels, drawn from shapSeed, forward passes only, shapPerms (cells + 1) of them per clip -- and writes a
    further pickle of records with 'ShapHeatMap' [T,H,W], 'ShapCells' and 'ShapStderr' [gt,gh,gw], 'ShapFrames' [T],
    'shap_total', 'n_perms', 'seed'.
    camKinds (an extension as well; with doGradCam) lists further members of the activation-map family --
    'gradcam++', 'xgradcam', 'hirescam', 'layercam' -- computed in the same call as Grad-CAM on camTarget (default: the
    Grad-CAM target, then from the one forward and backward), returned per clip batch as cam_<kind>, written to a
    further pickle (CamFamily in place of GradCam) of records with one [T,H,W] map per kind, and ranked by doCurves.
    doCurves (an extension as well, whatever the maskType; freeze only) also runs the deletion and insertion curves of
    every attribution the call produced -- the cells of curveGrid (gt, gh, gw) (default (T, 1, 1): the frames, ranked by
    the frame profiles; with a spatial grid by the [T,H,W] maps), blurred by curveSigma input pixels, frozen or released
    curveStep at a time in the order each attribution ranks them -- and writes a further pickle of records with 'grid',
    'step' and per method a dict of 'ranks', 'deletion', 'insertion', 'del_auc', 'ins_auc', 'del_auc_norm',
    'ins_auc_norm' ('random': the expected curves of a random order, when doShapley ran on the same grid)."""
    return ivf_find_masks.find_masks_impl(
        dat_loader, model, hyper_params, lam1, lam2, N, temporalMaskType, classOI, verbose, doGradCam,
        runTempMask, flavour="smth", sub_dir=_state["sub_dir"],
        gradcam_size=(RESIZE_SIZE_HEIGHT, RESIZE_SIZE_WIDTH),
        mask_mode=maskType if maskType in ("combi", "spacetime", "stcombi") else "central",
        max_mask_length=maxMaskLength, mask_grid=maskGrid, mask_sigma=maskSigma, lam3=lam3, max_box=maxBox,
        do_intgrad=doIntGrad, ig_steps=igSteps, ig_baseline=igBaseline, do_rise=doRise, rise_masks=riseMasks,
        rise_p=riseProb, rise_grid=riseGrid, rise_sigma=riseSigma, rise_seed=riseSeed, do_smoothgrad=doSmoothGrad,
        sg_samples=sgSamples, sg_level=sgLevel, sg_seed=sgSeed, do_shapley=doShapley, shap_perms=shapPerms,
        shap_grid=shapGrid, shap_sigma=shapSigma, shap_seed=shapSeed, do_curves=doCurves, curve_grid=curveGrid,
        curve_sigma=curveSigma, curve_step=curveStep, cam_kinds=camKinds, cam_target=camTarget,
        do_scorecam=doScoreCam, scorecam_target=scoreCamTarget, scorecam_weights=scoreCamWeights,
        scorecam_perturb=scoreCamPerturb, scorecam_sigma=scoreCamSigma, scorecam_channels=scoreCamChannels,
        do_kernelshap=doKernelShap, kshap_samples=kshapSamples, kshap_grid=kshapGrid, kshap_sigma=kshapSigma,
        kshap_seed=kshapSeed, do_lime=doLime, lime_samples=limeSamples, lime_p=limeProb, lime_grid=limeGrid,
        lime_sigma=limeSigma, lime_seed=limeSeed, lime_width=limeWidth, lime_ridge=limeRidge)


def main(argv=None):
    args = utils.load_args(argv)
    config = utils.load_module(args.config).config
    cnn_def = importlib.import_module(config['conv_model'])
    device, device_ids = utils.setup_cuda_devices(args)
    torch.cuda.set_device(device)
    print(" > Using device: {}".format(device.type))
    print(" > Active GPU ids: {}".format(device_ids))
    _state["sub_dir"] = args.subDir
    msl = args.mod_stride_layers if args.mod_stride_layers is not None else config.get('stride_mod_layers', "")
    model = cnn_def.Model(config['num_classes'], last_stride=1, stride_mod_layers=msl, softMax=1).to(device)  # smth:55-58
    ivf_find_masks.load_checkpoint_into(model, args.checkpoint)
    lam1 = args.lam1 if args.lam1 is not None else 0.01            # smth:106-113
    lam2 = args.lam2 if args.lam2 is not None else 0.02
    N = args.optIter if args.optIter is not None else 300           # smth:116-119
    if args.synthetic:
        loader = ivf_find_masks.SyntheticLoader(args.synthetic, config['batch_size'],
                                                (3, config['clip_size'], 224, 224), config['num_classes'])
    else:
        import ivf_ingest
        loader = ivf_ingest.JpegFolderLoader(config['data_folder'] + "/validation/", clip_size=config['clip_size'],
                                             batch_size=config['batch_size'], layout="smth",
                                             drop_last=True, device=device)     # val_loader, smth:71-77
    config.setdefault("gradCamType", args.gradCamType)
    find_masks(loader, model, config, lam1, lam2, N, "central", config.get("maskPerturbType", "freeze"),
               classOI=args.subsetFile, doGradCam=True, runTempMask=True)


if __name__ == '__main__':
    main()

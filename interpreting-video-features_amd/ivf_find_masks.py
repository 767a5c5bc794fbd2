"""Shared body of the two drop-in drivers (FindMasksComparison_I3D_{smth,KTH}.py).

Reproduces the INTENDED behaviour of the reference's `find_masks` (neither
published driver runs as-is): per clip, baseline scores ->
init_mask('central') -> N Adam iterations -> reverse score -> Grad-CAM, result
dicts with the reference's keys, the two pickles and the per-clip
ClassScore{Freeze,Reverse}case<id>.txt files (smth:222-251, 272-277, 307-313;
KTH:273-303, 330-334, 372-378).  All clips of a loader batch are searched
together with per-clip masks.
"""
import csv
import os
import pickle

import numpy as np
import torch

import ivf_lib as L
import ivf_search


def _class_filter(classOI):
    """smth:147,173-175: csv whose columns are class ids and cells clip ids."""
    if classOI is None:
        return None
    table = {}
    with open(classOI, newline='') as f:
        rows = list(csv.reader(f))
    header = rows[0]
    for j, key in enumerate(header):
        vals = set()
        for r in rows[1:]:
            if j < len(r) and r[j] != '':
                try:
                    vals.add(int(float(r[j])))
                except ValueError:
                    pass
        table[str(key)] = vals
    return table


def _unwrap(model):
    return model.module if hasattr(model, "module") and not hasattr(model, "_engine_for") else model


def find_masks_impl(dat_loader, model, hyper_params, lam1, lam2, N, temporalMaskType="freeze", classOI=None,
                    verbose=True, doGradCam=False, runTempMask=True, flavour="smth", sub_dir="run0",
                    results_path="results/", gradcam_size=None, write_files=True, device=None, visualise=True,
                    mask_mode="central", max_mask_length=None, blob_batch=32, mask_grid=None, mask_sigma=None, lam3=None,
                    max_box=None, do_intgrad=False, ig_steps=32, ig_baseline="frozen", do_rise=False, rise_masks=1024,
                    rise_p=0.5, rise_grid=None, rise_sigma=None, rise_seed=0, do_smoothgrad=False, sg_samples=32,
                    sg_level=0.15, sg_seed=0, do_shapley=False, shap_perms=64, shap_grid=None, shap_sigma=None,
                    shap_seed=0, do_curves=False, curve_grid=None, curve_sigma=None, curve_step=1, cam_kinds=(),
                    cam_target=None, do_scorecam=False, scorecam_target=None, scorecam_weights="increase",
                    scorecam_perturb="freeze", scorecam_sigma=None, scorecam_channels=None, do_kernelshap=False,
                    kshap_samples=256, kshap_grid=None, kshap_sigma=None, kshap_seed=0, do_lime=False, lime_samples=1024,
                    lime_p=0.5, lime_grid=None, lime_sigma=None, lime_seed=0, lime_width=0.25, lime_ridge=1.0):
    """do_kernelshap, do_lime (the drivers' doKernelShap and doLime, extensions: DESIGN 20) also fit a linear surrogate
    of the target's score drop in the frozen cells of kshap_grid / lime_grid (gt, gh, gw) (default (T, 1, 1): the
    frames; blurred by kshap_sigma / lime_sigma input pixels; forward passes only, the fit in fp64 on the device):
    KernelSHAP on kshap_samples paired coalitions drawn from kshap_seed, LIME on lime_samples Bernoulli(lime_p) rows
    drawn from lime_seed with kernel width lime_width and ridge lime_ridge.  Each writes a further list of records --
    true_class, pred_class, video_id, KshapHeatMap [T,H,W], KshapCells [gt,gh,gw], KshapFrames [T], kshap_total,
    kshap_ok, kshap_r2, n_samples, seed; and LimeHeatMap, LimeCells, LimeFrames, lime_intercept, lime_ok, lime_r2,
    n_samples, seed -- to a pickle named like the Grad-CAM one with KernelShap / Lime in place of GradCam; with the
    strips on, a further set of heat-map strips (folders `kernelshap` and `lime` beside `combined`) blends max(map, 0)
    normalised per frame, as Shapley's; the plan holds at least blob_batch clips so that the rows of a loader batch fill
    it; do_curves ranks the maps under 'kshap' and 'lime'.  Off, nothing changes.
    do_scorecam (the drivers' doScoreCam, an extension: DESIGN 19) also runs Score-CAM of the target's score on
    scorecam_target (default: the Grad-CAM target; scorecam_channels = (first, count) a window of its channels, each
    normalised, expanded with a blur of scorecam_sigma input pixels and applied as scorecam_perturb 'freeze' or 'blank',
    weighted as scorecam_weights 'increase' or 'softmax'; forward passes only) and writes a further list of records --
    true_class, pred_class, video_id, ScoreCamHeatMap [frames,H,W], ScoreCamWeights, ScoreCamValid [nc], score_base, layer,
    weights, perturb -- to a pickle named like the Grad-CAM one with ScoreCam in place of GradCam; with the strips on, a
    further set of heat-map strips (folder `scorecam` beside `combined`) blends the map; its plan holds at least
    blob_batch clips so that the channel rows of a loader batch fill it; do_curves ranks the map under 'scorecam'.  The
    multi-GPU record gather (ivf_shard) does not carry these records.  Off, nothing changes.
    cam_kinds (the drivers' camKinds, an extension: DESIGN 18; with doGradCam) also computes the listed members of the
    Grad-CAM family ('gradcam++', 'xgradcam', 'hirescam', 'layercam') on cam_target (default: the Grad-CAM target, then
    from Grad-CAM's own forward and backward) and writes a further list of records -- true_class, pred_class, video_id
    and one [T,H,W] float32 map per kind -- to a pickle named like the Grad-CAM one with CamFamily in place of GradCam;
    do_curves ranks them under the kind's name.  Empty, nothing changes.
    do_curves (the drivers' doCurves, an extension: DESIGN 17) also runs the deletion and insertion curves of every
    attribution the call produced (ivf_search.MaskSearch: the frame profiles on the default frame grid, the [T,H,W] maps
    on a spatial curve_grid; curve_sigma the blur in input pixels, curve_step cells per forward; freeze only) and writes
    a further list of records -- true_class, pred_class, video_id, grid, step, and per method ('time_mask' or
    'st_mask', 'gradcam', 'ig', 'rise', 'sg', 'shap', and 'random' when Shapley ran on the same grid and sigma) a dict
    of ranks [P] (None for 'random'), deletion, insertion [J+1], del_auc, ins_auc, del_auc_norm, ins_auc_norm -- to a
    pickle named like the Grad-CAM one with Curves in place of GradCam; its plan holds at least blob_batch clips so that
    the rows of a loader batch fill it.  The multi-GPU record gather (ivf_shard) does not carry these records.  Off,
    nothing changes.
    do_shapley (the drivers' doShapley, an extension: DESIGN 16) also runs Shapley value sampling of the target's score
    (shap_perms permutations of the cells of shap_grid (gt, gh, gw), default (T, 1, 1): the frames; blurred by shap_sigma
    input pixels, drawn from shap_seed; forward passes only) and writes a further list of records -- true_class,
    pred_class, video_id, ShapHeatMap [T,H,W], ShapCells, ShapStderr [gt,gh,gw], ShapFrames [T], shap_total, n_perms, seed
    -- to a pickle named like the Grad-CAM one with Shapley in place of GradCam; with the strips on, a further set of
    heat-map strips (folder `shapley` beside `combined`) blends max(shap_map, 0) normalised per frame; its plan holds at
    least blob_batch clips so that the rows of a loader batch fill it.  Off, nothing changes.
    do_smoothgrad (the drivers' doSmoothGrad, an extension: DESIGN 15) also runs SmoothGrad, SmoothGrad^2 and VarGrad
    of the target's score (sg_samples noisy copies of each clip, noise of standard deviation sg_level * (max - min) of
    the clip drawn from sg_seed, one forward and backward each) and writes a further list of records -- true_class,
    pred_class, video_id, SGHeatMap, SGSqHeatMap, SGVarHeatMap [T,H,W], SGFrames [T], sigma, n_samples, level, seed -- to
    a pickle named like the Grad-CAM one with SmoothGrad in place of GradCam; with the strips on, a further set of
    heat-map strips (folder `smoothgrad` beside `combined`) blends sg_map scaled per frame; its plan holds at least
    blob_batch clips so that the samples of a loader batch fill it.  Off, nothing changes.
    do_rise (the drivers' doRise, an extension: DESIGN 14) also runs RISE random-mask saliency of the target's score
    (rise_masks masks on rise_grid (gt, gh, gw), each cell frozen with probability rise_p, blurred by rise_sigma input
    pixels, drawn from rise_seed; forward passes only) and writes a further list of records -- true_class, pred_class,
    video_id, RiseHeatMap [T,H,W], RiseCells [gt,gh,gw], RiseCount, RiseFrames [T], rise_mean_drop, n_masks, p, seed --
    to a pickle named like the Grad-CAM one with Rise in place of GradCam; with the strips on, a further set of
    heat-map strips (folder `rise` beside `combined`) blends max(rise_map, 0) normalised per frame; its plan holds at
    least blob_batch clips so that the masks of a loader batch fill it.  Off, nothing changes.
    do_intgrad (the drivers' doIntGrad, an extension: DESIGN 13) also runs Integrated Gradients of the target's score
    (ig_steps midpoint nodes from ig_baseline 'frozen' or 'constant') and writes a third list of records -- true_class,
    pred_class, video_id, IGHeatMap [T,H,W], IGFrames [T], ig_total, ig_gap, score_base -- to a third pickle named like
    the Grad-CAM one with IntGrad in place of GradCam; with the strips on, a second set of heat-map strips (folder
    `intgrad` beside `combined`) blends max(ig_map, 0) normalised per frame.  Off, nothing changes.
    mask_mode 'stcombi' (the drivers' maskType='stcombi', an extension: DESIGN 12) scores every one-box space-time
    mask (one temporal blob of length <= max_mask_length times one rectangle of at most max_box grid cells) and keeps the
    minimiser of the spacetime loss; its plan holds at least blob_batch clips, its records also carry st_mask (binary),
    box_start, box_length, box_rows (i0, bh), box_cols (j0, bw) and box_drop [T,gh,gw], and the strips and PNGs are
    made from the expanded box as for 'spacetime'.
    mask_mode 'spacetime' (the drivers' maskType='spacetime', an extension: DESIGN 11) searches a mask per frame
    and grid cell (mask_grid, mask_sigma, lam3: see ivf_search.MaskSearch); its records also carry st_mask
    [T,gh,gw], the heat-map strips blend the expanded mask where they blend the Grad-CAM map otherwise, and the KTH
    flavour's perturbed-frame PNGs show the per-pixel freeze that was searched (the mark in their corner is time_mask).
    mask_mode 'combi' (the drivers' maskType='combi', smth:137-141) replaces init_mask + Adam by the exhaustive
    one-blob search over masks of length <= max_mask_length; its plan holds at least blob_batch clips so that the
    candidates of a loader batch fill it.  Its records also carry blob_start, blob_length and blob_scores."""
    net = _unwrap(model)
    net.eval()                                                      # smth:145
    flt = _class_filter(classOI)
    masks, time_results, cam_results, ig_results, rise_results, sg_results = [], [], [], [], [], []
    shap_results, curve_results, fam_results, scorecam_results = [], [], [], []
    kshap_results, lime_results = [], []
    cam_kinds = tuple(cam_kinds) if doGradCam else ()
    if write_files and not os.path.exists(results_path):
        os.makedirs(results_path)
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    for i, (sequence, label, video_id) in enumerate(dat_loader):
        if i % 50 == 0 and verbose:
            print("on idx: ", i)
        x = L.f32c(sequence.to(dev))                                # smth:158
        labels = torch.as_tensor(label).reshape(-1)
        ids = [v.item() if torch.is_tensor(v) else v for v in video_id] if not isinstance(video_id, str) else [video_id]
        keep = []
        for bi in range(x.shape[0]):                                # smth:166-175
            tc = str(int(labels[bi]))
            if flt is None or (tc in flt and int(ids[bi]) in flt[tc]):
                keep.append(bi)
        if not keep:
            continue
        xs = x[keep].contiguous()
        eng = net._engine_for(xs, min_batch=blob_batch) if mask_mode in ("combi", "stcombi") or do_rise or do_smoothgrad \
            or do_shapley or do_curves or do_scorecam or do_kernelshap or do_lime else net._engine_for(xs)
        search = ivf_search.MaskSearch(eng, lam1, lam2, N, temporalMaskType, threshold=0.9, lr=0.2,
                                       grad_cam_type=hyper_params.get("gradCamType", "guessed"),
                                       do_gradcam=doGradCam, run_temp_mask=runTempMask,
                                       normalize_per_frame=True, gradcam_size=gradcam_size, mask_mode=mask_mode,
                                       max_mask_length=max_mask_length, mask_grid=mask_grid, mask_sigma=mask_sigma,
                                       lam3=lam3, max_box=max_box, do_intgrad=do_intgrad, ig_steps=ig_steps,
                                       ig_baseline=ig_baseline, do_rise=do_rise, rise_masks=rise_masks, rise_p=rise_p,
                                       rise_grid=rise_grid, rise_sigma=rise_sigma, rise_seed=rise_seed,
                                       do_smoothgrad=do_smoothgrad, sg_samples=sg_samples, sg_level=sg_level,
                                       sg_seed=sg_seed, do_shapley=do_shapley, shap_perms=shap_perms, shap_grid=shap_grid,
                                       shap_sigma=shap_sigma, shap_seed=shap_seed, do_curves=do_curves,
                                       curve_grid=curve_grid, curve_sigma=curve_sigma, curve_step=curve_step,
                                       cam_kinds=cam_kinds, cam_target=cam_target, do_scorecam=do_scorecam,
                                       scorecam_target=scorecam_target, scorecam_weights=scorecam_weights,
                                       scorecam_perturb=scorecam_perturb, scorecam_sigma=scorecam_sigma,
                                       scorecam_channels=scorecam_channels, do_kernelshap=do_kernelshap,
                                       kshap_samples=kshap_samples, kshap_grid=kshap_grid, kshap_sigma=kshap_sigma,
                                       kshap_seed=kshap_seed, do_lime=do_lime, lime_samples=lime_samples, lime_p=lime_p,
                                       lime_grid=lime_grid, lime_sigma=lime_sigma, lime_seed=lime_seed,
                                       lime_width=lime_width, lime_ridge=lime_ridge)
        res = search.run(xs, labels[keep])
        host = {k: v.detach().cpu() for k, v in res.items()
                if k not in ("gradcam", "box_scores", "ig_map", "rise_map", "sg_map", "sg_sq_map", "sg_var_map", "shap_map",
                            "scorecam_map", "kshap_map", "lime_map")}
        spacetime = runTempMask and mask_mode in ("spacetime", "stcombi")
        st_maps = eng.st_expand(res["st_mask"], search.st_grid(xs), mask_sigma) if spacetime and write_files and visualise \
            else None
        st_pert = eng.st_freeze(xs, st_maps) if st_maps is not None and flavour != "smth" else None   # what was searched
        if doGradCam:
            host["gradcam"] = res["gradcam"].detach().cpu()
        ig_heat = None
        if do_intgrad:
            host["ig_map"] = res["ig_map"].detach().cpu()
            if runTempMask and write_files and visualise:
                # max(ig_map, 0) scaled to [0,1] per frame, the range ivf_viz_blend takes; a frame without a positive
                # attribution (frame 0 under 'frozen') stays all zero
                pos = res["ig_map"].clamp_min(0.0)
                top = pos.amax(dim=(2, 3), keepdim=True)
                ig_heat = torch.where(top > 0, pos / torch.where(top > 0, top, torch.ones_like(top)), torch.zeros_like(pos))
        rise_heat = None
        if do_rise:
            host["rise_map"] = res["rise_map"].detach().cpu()
            if runTempMask and write_files and visualise:
                # as ig_heat: max(rise_map, 0) scaled to [0,1] per frame; a frame without a positive drop stays all zero
                pos = res["rise_map"].clamp_min(0.0)
                top = pos.amax(dim=(2, 3), keepdim=True)
                rise_heat = torch.where(top > 0, pos / torch.where(top > 0, top, torch.ones_like(top)), torch.zeros_like(pos))
        sg_heat = None
        if do_smoothgrad:
            for k in ("sg_map", "sg_sq_map", "sg_var_map"):
                host[k] = res[k].detach().cpu()
            if runTempMask and write_files and visualise:
                # as ig_heat: sg_map (non-negative) scaled to [0,1] per frame; a frame without a gradient stays all zero
                pos = res["sg_map"].clamp_min(0.0)
                top = pos.amax(dim=(2, 3), keepdim=True)
                sg_heat = torch.where(top > 0, pos / torch.where(top > 0, top, torch.ones_like(top)), torch.zeros_like(pos))
        shap_heat = None
        if do_shapley:
            host["shap_map"] = res["shap_map"].detach().cpu()
            if runTempMask and write_files and visualise:
                # as rise_heat: max(shap_map, 0) scaled to [0,1] per frame; a frame without a positive value stays all zero
                pos = res["shap_map"].clamp_min(0.0)
                top = pos.amax(dim=(2, 3), keepdim=True)
                shap_heat = torch.where(top > 0, pos / torch.where(top > 0, top, torch.ones_like(top)), torch.zeros_like(pos))
        lin_heat = {}
        for on, name in ((do_kernelshap, "kshap"), (do_lime, "lime")):
            if on:
                host[name + "_map"] = res[name + "_map"].detach().cpu()
                if runTempMask and write_files and visualise:
                    # as shap_heat: max(map, 0) scaled to [0,1] per frame; a frame without a positive value (and a map
                    # that is NaN because its fit was refused) stays all zero
                    pos = torch.nan_to_num(res[name + "_map"], nan=0.0).clamp_min(0.0)
                    top = pos.amax(dim=(2, 3), keepdim=True)
                    lin_heat[name] = torch.where(top > 0, pos / torch.where(top > 0, top, torch.ones_like(top)),
                                                 torch.zeros_like(pos))
        scorecam_heat = None
        if do_scorecam:
            host["scorecam_map"] = res["scorecam_map"].detach().cpu()
            if runTempMask and write_files and visualise and res["scorecam_map"].shape[1] == xs.shape[2]:
                # the map is normalised to [0,1] as the Grad-CAM map is; a constant slice (NaN there) stays all zero
                scorecam_heat = torch.nan_to_num(res["scorecam_map"], nan=0.0).clamp(0.0, 1.0)
        for j, bi in enumerate(keep):
            true_class = int(labels[bi])
            pred = int(host["pred_class"][j])
            vid = ids[bi]
            gs = float(host["original_score_guess"][j])
            cs = float(host["original_score_true"][j])
            if runTempMask:
                tm = host["time_mask"][j].numpy()
                fz, rv = float(host["freeze_score"][j]), float(host["reverse_score"][j])
                if write_files:
                    gs_name = int(gs) if flavour == "smth" else gs     # smth:218 casts the score with int()
                    d = os.path.join("cam_saved_images", sub_dir, str(true_class),
                                     str(vid) + "g_" + str(pred) + "_gs%5.4f" % gs_name + "_cs%5.4f" % cs, "combined")
                    os.makedirs(d, exist_ok=True)
                    with open(os.path.join(d, "ClassScoreFreezecase" + str(vid) + ".txt"), "w+") as f:
                        f.write(str(fz))
                    with open(os.path.join(d, "ClassScoreReversecase" + str(vid) + ".txt"), "w+") as f:
                        f.write(str(rv))
                time_results.append({'true_class': true_class, 'pred_class': pred, 'video_id': vid,
                                     'time_mask': tm,
                                     'original_score_guess': int(gs) if flavour == "smth" else gs,
                                     'original_score_true': cs, 'freeze_score': fz, 'reverse_score': rv})
                if mask_mode == "combi":
                    time_results[-1].update(blob_start=int(host["blob"][j, 0]), blob_length=int(host["blob"][j, 1]),
                                            blob_scores=host["blob_scores"][j].numpy())
                if spacetime:
                    time_results[-1].update(st_mask=host["st_mask"][j].numpy())
                if runTempMask and mask_mode == "stcombi":
                    bx = [int(v) for v in host["box"][j]]
                    time_results[-1].update(box_start=bx[0], box_length=bx[1], box_rows=(bx[2], bx[3]),
                                            box_cols=(bx[4], bx[5]), box_drop=host["box_drop"][j].numpy())
                tmask = res["time_mask"][j].clone()     # the clip's own [T] tensor, as the reference's time_mask
                if verbose:
                    print("resulting mask is: ", tmask)
            if doGradCam:
                cam_results.append({'true_class': true_class, 'pred_class': pred,
                                    'video_id': int(vid) if flavour == "smth" else vid,
                                    'GCHeatMap': host["gradcam"][j].numpy().astype(np.float32)})
            if cam_kinds:
                fam_results.append({'true_class': true_class, 'pred_class': pred,
                                    'video_id': int(vid) if flavour == "smth" else vid,
                                    **{k: host["cam_" + k][j].numpy().astype(np.float32) for k in cam_kinds}})
            if do_intgrad:
                ig_results.append({'true_class': true_class, 'pred_class': pred,
                                   'video_id': int(vid) if flavour == "smth" else vid,
                                   'IGHeatMap': host["ig_map"][j].numpy().astype(np.float32),
                                   'IGFrames': host["ig_frames"][j].numpy().astype(np.float32),
                                   'ig_total': float(host["ig_total"][j]), 'ig_gap': float(host["ig_gap"][j]),
                                   'score_base': float(host["ig_score_base"][j])})
            if do_rise:
                rise_results.append({'true_class': true_class, 'pred_class': pred,
                                     'video_id': int(vid) if flavour == "smth" else vid,
                                     'RiseHeatMap': host["rise_map"][j].numpy().astype(np.float32),
                                     'RiseCells': host["rise_cells"][j].numpy().astype(np.float32),
                                     'RiseCount': host["rise_count"][j].numpy(),
                                     'RiseFrames': host["rise_frames"][j].numpy().astype(np.float32),
                                     'rise_mean_drop': float(host["rise_mean_drop"][j]),
                                     'n_masks': int(rise_masks), 'p': float(rise_p), 'seed': int(rise_seed)})
            if do_smoothgrad:
                sg_results.append({'true_class': true_class, 'pred_class': pred,
                                   'video_id': int(vid) if flavour == "smth" else vid,
                                   'SGHeatMap': host["sg_map"][j].numpy().astype(np.float32),
                                   'SGSqHeatMap': host["sg_sq_map"][j].numpy().astype(np.float32),
                                   'SGVarHeatMap': host["sg_var_map"][j].numpy().astype(np.float32),
                                   'SGFrames': host["sg_frames"][j].numpy().astype(np.float32),
                                   'sigma': float(host["sg_sigma"][j]), 'n_samples': int(sg_samples),
                                   'level': float(sg_level), 'seed': int(sg_seed)})
            if do_shapley:
                shap_results.append({'true_class': true_class, 'pred_class': pred,
                                     'video_id': int(vid) if flavour == "smth" else vid,
                                     'ShapHeatMap': host["shap_map"][j].numpy().astype(np.float32),
                                     'ShapCells': host["shap_cells"][j].numpy().astype(np.float32),
                                     'ShapStderr': host["shap_stderr"][j].numpy().astype(np.float32),
                                     'ShapFrames': host["shap_frames"][j].numpy().astype(np.float32),
                                     'shap_total': float(host["shap_total"][j]),
                                     'n_perms': int(shap_perms), 'seed': int(shap_seed)})
            if do_kernelshap:
                kshap_results.append({'true_class': true_class, 'pred_class': pred,
                                      'video_id': int(vid) if flavour == "smth" else vid,
                                      'KshapHeatMap': host["kshap_map"][j].numpy().astype(np.float32),
                                      'KshapCells': host["kshap_cells"][j].numpy().astype(np.float32),
                                      'KshapFrames': host["kshap_frames"][j].numpy().astype(np.float32),
                                      'kshap_total': float(host["kshap_total"][j]), 'kshap_ok': int(host["kshap_ok"][j]),
                                      'kshap_r2': float(host["kshap_r2"][j]),
                                      'n_samples': int(kshap_samples), 'seed': int(kshap_seed)})
            if do_lime:
                lime_results.append({'true_class': true_class, 'pred_class': pred,
                                     'video_id': int(vid) if flavour == "smth" else vid,
                                     'LimeHeatMap': host["lime_map"][j].numpy().astype(np.float32),
                                     'LimeCells': host["lime_cells"][j].numpy().astype(np.float32),
                                     'LimeFrames': host["lime_frames"][j].numpy().astype(np.float32),
                                     'lime_intercept': float(host["lime_intercept"][j]), 'lime_ok': int(host["lime_ok"][j]),
                                     'lime_r2': float(host["lime_r2"][j]),
                                     'n_samples': int(lime_samples), 'seed': int(lime_seed)})
            if do_scorecam:
                scorecam_results.append({'true_class': true_class, 'pred_class': pred,
                                         'video_id': int(vid) if flavour == "smth" else vid,
                                         'ScoreCamHeatMap': host["scorecam_map"][j].numpy().astype(np.float32),
                                         'ScoreCamWeights': host["scorecam_weights"][j].numpy().astype(np.float32),
                                         'ScoreCamValid': host["scorecam_valid"][j].numpy().astype(bool),
                                         'score_base': float(host["scorecam_score_base"][j]), 'layer': scorecam_target,
                                         'weights': scorecam_weights, 'perturb': scorecam_perturb})
            if do_curves:
                T_ = xs.shape[2]
                rec = {'true_class': true_class, 'pred_class': pred, 'video_id': int(vid) if flavour == "smth" else vid,
                       'grid': (T_, 1, 1) if curve_grid is None else tuple(int(v) for v in curve_grid),
                       'step': int(curve_step)}
                for key in host:
                    if key.startswith("curves_") and key.endswith("_deletion"):
                        m = key[len("curves_"):-len("_deletion")]
                        rk = host.get(f"curves_{m}_ranks")
                        rec[m] = {'ranks': None if rk is None else rk[j].numpy().astype(np.int64) & 0xFFFF,
                                  'deletion': host[key][j].numpy().astype(np.float32),
                                  'insertion': host[f"curves_{m}_insertion"][j].numpy().astype(np.float32)}
                        for k in ("del_auc", "ins_auc", "del_auc_norm", "ins_auc_norm"):
                            rec[m][k] = float(host[f"curves_{m}_{k}"][j])
                curve_results.append(rec)
            if runTempMask and write_files and visualise:
                # smth:296-303 / KTH:354-367: heat-map strips with the mask dot row for both perturbation
                # types (the dot row snaps a host copy: `tmask` keeps its sigmoid values, as the reference's
                # CUDA time_mask does), then for KTH the perturbed frames as PNGs of the SOFT mask
                import visualisation as viz
                if doGradCam or st_maps is not None:
                    heat = st_maps[j] if st_maps is not None else res["gradcam"][j]
                    for kind in ("freeze", "reverse"):
                        viz.create_image_arrays(xs, heat, tmask, j, kind, d, str(vid), 0, xs.shape[4], xs.shape[3])
                if ig_heat is not None:
                    for kind in ("freeze", "reverse"):
                        viz.create_image_arrays(xs, ig_heat[j], tmask, j, kind, os.path.join(os.path.dirname(d), "intgrad"),
                                                str(vid), 0, xs.shape[4], xs.shape[3])
                if rise_heat is not None:
                    for kind in ("freeze", "reverse"):
                        viz.create_image_arrays(xs, rise_heat[j], tmask, j, kind, os.path.join(os.path.dirname(d), "rise"),
                                                str(vid), 0, xs.shape[4], xs.shape[3])
                if sg_heat is not None:
                    for kind in ("freeze", "reverse"):
                        viz.create_image_arrays(xs, sg_heat[j], tmask, j, kind,
                                                os.path.join(os.path.dirname(d), "smoothgrad"), str(vid), 0, xs.shape[4],
                                                xs.shape[3])
                if shap_heat is not None:
                    for kind in ("freeze", "reverse"):
                        viz.create_image_arrays(xs, shap_heat[j], tmask, j, kind, os.path.join(os.path.dirname(d), "shapley"),
                                                str(vid), 0, xs.shape[4], xs.shape[3])
                for name, folder in (("kshap", "kernelshap"), ("lime", "lime")):
                    if name in lin_heat:
                        for kind in ("freeze", "reverse"):
                            viz.create_image_arrays(xs, lin_heat[name][j], tmask, j, kind,
                                                    os.path.join(os.path.dirname(d), folder), str(vid), 0, xs.shape[4],
                                                    xs.shape[3])
                if scorecam_heat is not None:
                    for kind in ("freeze", "reverse"):
                        viz.create_image_arrays(xs, scorecam_heat[j], tmask, j, kind,
                                                os.path.join(os.path.dirname(d), "scorecam"), str(vid), 0, xs.shape[4],
                                                xs.shape[3])
                if flavour != "smth":
                    import mask as _mask
                    pert = st_pert[j] if st_pert is not None else _mask.perturb_sequence(xs, tmask, temporalMaskType)[j]
                    viz.vizualize_results(xs[j], pert, tmask,
                                          rootDir=d, case=str(vid), markImgs=True, iterTest=False)
            # smth:303 appends only when both Grad-CAM and the mask search ran; KTH:367 whenever the search ran
            if runTempMask and (doGradCam or flavour != "smth"):
                masks.append(tmask)
    if write_files:
        if flavour == "smth":                                       # smth:307-313
            tname = "allTimeMaskResults_" + sub_dir + "_" + str(classOI) + "_" + ".p"
            gname = "allGradCamResults_" + sub_dir + "_" + str(classOI) + "_" + ".p"
        else:                                                       # KTH:372-378
            tname = "I3d_KTH_allTimeMaskResults_original_" + sub_dir + ".p"
            gname = "I3d_KTH_allGradCamResults_original_" + sub_dir + ".p"
        with open(os.path.join(results_path, tname.replace(os.sep, "_")), "wb") as f:
            pickle.dump(time_results, f)
        with open(os.path.join(results_path, gname.replace(os.sep, "_")), "wb") as f:
            pickle.dump(cam_results, f)
        if cam_kinds:
            with open(os.path.join(results_path, gname.replace("GradCam", "CamFamily").replace(os.sep, "_")), "wb") as f:
                pickle.dump(fam_results, f)
        if do_intgrad:
            with open(os.path.join(results_path, gname.replace("GradCam", "IntGrad").replace(os.sep, "_")), "wb") as f:
                pickle.dump(ig_results, f)
        if do_rise:
            with open(os.path.join(results_path, gname.replace("GradCam", "Rise").replace(os.sep, "_")), "wb") as f:
                pickle.dump(rise_results, f)
        if do_smoothgrad:
            with open(os.path.join(results_path, gname.replace("GradCam", "SmoothGrad").replace(os.sep, "_")), "wb") as f:
                pickle.dump(sg_results, f)
        if do_shapley:
            with open(os.path.join(results_path, gname.replace("GradCam", "Shapley").replace(os.sep, "_")), "wb") as f:
                pickle.dump(shap_results, f)
        if do_kernelshap:
            with open(os.path.join(results_path, gname.replace("GradCam", "KernelShap").replace(os.sep, "_")), "wb") as f:
                pickle.dump(kshap_results, f)
        if do_lime:
            with open(os.path.join(results_path, gname.replace("GradCam", "Lime").replace(os.sep, "_")), "wb") as f:
                pickle.dump(lime_results, f)
        if do_scorecam:
            with open(os.path.join(results_path, gname.replace("GradCam", "ScoreCam").replace(os.sep, "_")), "wb") as f:
                pickle.dump(scorecam_results, f)
        if do_curves:
            with open(os.path.join(results_path, gname.replace("GradCam", "Curves").replace(os.sep, "_")), "wb") as f:
                pickle.dump(curve_results, f)
    find_masks_impl.last_results = (time_results, cam_results)
    find_masks_impl.last_ig_results = ig_results
    find_masks_impl.last_rise_results = rise_results
    find_masks_impl.last_sg_results = sg_results
    find_masks_impl.last_shap_results = shap_results
    find_masks_impl.last_kshap_results = kshap_results
    find_masks_impl.last_lime_results = lime_results
    find_masks_impl.last_curve_results = curve_results
    find_masks_impl.last_cam_family_results = fam_results
    find_masks_impl.last_scorecam_results = scorecam_results
    return masks


class SyntheticLoader:
    """Stand-in for ImLoader/KTHImLoader batches (data_loader_jpg.py:23-41): yields
    (sequence [B,3,T,H,W] float 0..255, label [B], video_id list) from ivf_recipe."""

    def __init__(self, n_clips, batch_size, shape, num_classes, first_id=0):
        self.n, self.bs, self.shape, self.k, self.first = n_clips, batch_size, shape, num_classes, first_id

    def __iter__(self):
        import ivf_recipe as R
        for s in range(0, self.n - self.n % self.bs if self.n >= self.bs else self.n, self.bs):
            ids = list(range(self.first + s, self.first + min(s + self.bs, self.n)))
            seq = torch.from_numpy(np.stack([R.clip(c, *self.shape) for c in ids]))
            yield seq, torch.tensor([R.label(c, self.k) for c in ids]), [str(c) for c in ids]


def load_checkpoint_into(model, checkpoint_path):
    """smth:89-103: a missing checkpoint is a printed warning, not an error."""
    if checkpoint_path and os.path.isfile(checkpoint_path):
        print(" > Loading checkpoint '{}'".format(checkpoint_path))
        ck = torch.load(checkpoint_path, map_location="cpu")
        _unwrap(model).load_state_dict(ck['state_dict'] if 'state_dict' in ck else ck)
        print(" > Loaded checkpoint '{}' (epoch {})".format(checkpoint_path, ck.get('epoch', '?')))
        return True
    print(" !#! No checkpoint found at '{}'".format(checkpoint_path))
    return False

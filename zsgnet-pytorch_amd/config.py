"""Configuration (reference `code/extended_config.py` + `configs/cfg.json`): the same ~40 flags with the same defaults,
addressable as cfg['k'] and cfg.k, and the same override rule (key must exist, value must keep its type;
extended_config.py:78-88).  yacs is not available offline, so this is a small dict subclass."""
import ast
import copy
from typing import Any, Dict

DEFAULTS: Dict[str, Any] = {
    # configs/cfg.json:1-43
    "ds_to_use": "refclef", "bs": 16, "nw": 4, "bsv": 16, "nwv": 4, "lr": 1e-4, "devices": 0, "opt_fn": "Adam",
    # opt_fn: "Adam" / "AdamW" / "SGD" / "LAMB" (optim.make_opt_fn; LAMB: betas, eps, weight_decay, see lamb_adapt_1d below); opt_fn_params: the keys of all three, each rule takes its own (betas, eps, amsgrad:
    # Adam / AdamW; momentum, dampening, nesterov: SGD; weight_decay: all).  The reference has betas alone (cfg.json)
    "opt_fn_params": {"betas": [0.9, 0.99], "eps": 1e-8, "weight_decay": 0.0, "amsgrad": False, "momentum": 0.0, "dampening": 0.0,
                      "nesterov": False},
    "do_norm": False, "use_same_atb": True, "mdl_to_use": "retina",
    "resize_img": [300, 300], "tmp_path": "./tmp", "use_multi": True, "use_focal": True, "use_softmax": False,
    "alpha": 0.25, "gamma": 2, "ratios": "[1/2, 1, 2]", "scales": "[1, 2**(1/3), 2**(2/3)]", "scale_factor": 4,
    "emb_dim": 300, "matching_threshold": 0.6, "epochs": 10, "use_bidirectional": True, "lstm_dim": 128,
    "use_reduce_lr_plateau": True, "patience": 2, "reduce_factor": 0.1, "lamb_reg": 1, "resume_path": "",
    "resume": True, "load_opt": False, "strict_load": True, "load_normally": True, "acc_iou_threshold": 0.5,
    "use_lang": True, "use_img": True,
    # extended_config.py:13-21
    "device": "cuda", "local_rank": 0, "do_dist": False, "only_val": False, "only_test": False, "num_gpus": 1,
    # extensions of this build (documented in DESIGN.md)
    "resnet_arch": "resnet50",      # the reference hard-codes resnet50 (mdl.py:411); configs 1 and 5 need 18 / 101
    "pretrained_path": "",          # local checkpoint instead of the torchvision download
    "synthetic": True,              # synthetic batches instead of the CSV datasets
    "steps_per_epoch": 50,
    "word_vectors": "",             # .npz word-vector table (`words`, `vectors`) used when spaCy is not installed
    "gpu_img_normalise": True,      # images travel as uint8 HWC; /255 + NHWC4 on the GPU (bit-identical to the host path)
    "freeze_bn": False,             # every BatchNorm layer in eval mode while training (running statistics, no update): ZSGNet.freeze_batchnorm
    "clip_grad_norm": 0.0,          # > 0: Learner clips the trainable gradients to this total 2-norm before every step (optim.clip_grad_norm_); 0 = off
    "group_val_by_image": False,    # validation / test batches grouped by image file: each distinct image once + img_idx (ZSGNet's shared-image eval plan)
    "group_trn_by_image": False,    # training batches of bs queries over bs / trn_queries_per_image image slots + img_idx (ZSGNet.shared_training)
    "trn_queries_per_image": 4,     # ... queries per image slot (bs must be a multiple); rows of one file are cut into chunks of this size
    "sync_bn": False,              # with do_dist: BatchNorm statistics over the union of all ranks' batches (dist.convert_sync_batchnorm)
    "eval_topk": 1,                 # K > 1: in eval mode the evaluator also returns the K best NMS-filtered boxes per query and Acc@K (zsg_eval_topk)
    "eval_nms_thr": 0.5,            # ... a candidate is dropped when its IoU with a box already kept is > this
    "eval_pre_nms": 128,            # ... candidates per query (best scores first) that enter the NMS; K <= eval_pre_nms <= 512
    "lamb_adapt_1d": False,         # opt_fn "LAMB" (the large-batch rule: optim.FusedLAMB; reads betas, eps, weight_decay of opt_fn_params): by default tensors of >= 2 dimensions get the trust ratio and the 1-D ones (biases, BatchNorm scales / shifts) plain Adam steps without weight decay (optim.lamb_param_groups); True = one adaptive group of everything
    "lang_pool": "last",            # the query encoder's sentence vector, fixed at construction (ZSGNet.__init__): "last" = the reference's [h_fwd(len-1) | reverse cell on x[len-1]] (mdl.py:296-336); "final" = nn.LSTM's h_n [f_{len-1} | r_0] (the reverse direction reads the whole phrase); "mean" = the mean of the padded BiLSTM output over the valid tokens; "attn" = its softmax(w . o_t)-weighted sum with the extra parameter lang_pool.weight [1, lstm_out_dim] (zero-initialised: starts as "mean"); csrc/lstm_seq.hip
    "lang_fuse": "concat",          # how the sentence vector meets the image in the heads' first convolution, fixed at construction (ZSGNet.__init__): "concat" = the reference's concatenation (a purely additive effect: the vector is constant over the image); "film" = it also scales the convolution's feature part per query and channel, h1 = relu((1 + gamma) * conv(F, W0[:, :Cf]) + conv([lang | grid], W0[:, Cf:]) + bias) with gamma = W_gamma . we and one extra parameter per head stack, <head>.film.weight [256, lstm_out_dim] (zero-initialised: starts as "concat"); needs use_lang and use_img; csrc/film.hip; "words" = the scale becomes a function of the pixel: conv0's raw feature accumulator Y attends over the BiLSTM's per-token output o_t, alpha = softmax_t(Y[p] . W_key o_t / 16), gamma[p] = sum_t alpha_t W_value o_t, with two extra parameters per head stack, <head>.words.key.weight / <head>.words.value.weight [256, lstm_out_dim] (value zero-initialised: starts as "concat"); needs use_lang, use_img and lang_pool final / mean / attn; csrc/words.hip
    "head_ctx": "none",             # a global-context block behind the heads' first convolution, fixed at construction (ZSGNet.__init__): "none" = the reference's towers (an anchor sees a 13 x 13 cell window); "gc" (GCNet, Cao et al. 2019) = per query and pyramid level one attention-pooled vector of h1, c = sum_p softmax_p(k . x_p) x_p, through a bottleneck MLP (256 -> 64, LayerNorm, ReLU, 64 -> 256) and added to every pixel of h1, with seven extra parameters per head stack, <head>.gc.{key.weight, fc1.weight, fc1.bias, ln.weight, ln.bias, fc2.weight, fc2.bias} (fc2 zero-initialised: starts as "none"); csrc/gcblock.hip
    "warmup_iters": 0,              # W > 0: linear learning-rate warm-up — optimizer step k = 1..W runs at k / W of every group's base lr (the lr at prepare_optimizer), later steps leave the groups to the scheduler; a resume with load_opt continues from the checkpoint's num_it; 0 = off
    "ema_decay": 0.0,               # > 0: an exponential moving average of the weights, updated in every optimizer step (ema.ModelEma); 0 = off
    "ema_warmup": False,            # ... its decay ramps up as min(ema_decay, (1 + n) / (10 + n)) over the first updates
    "ema_eval": True,               # ... validation / testing (and with them the LR scheduler, best_met, the prediction files) use the average
    "aug_crop_min": 1.0,            # < 1 (in (0, 1]): training images are cropped to a random window of this fraction of each side at least, which always holds the box(es) (dat_loader.draw_augment); 1 = off
    "aug_brightness": 0.0,          # > 0: training images get a brightness factor from U(max(0, 1 - v), 1 + v) (dat_loader.augment_host; on the GPU with gpu_img_resize); 0 = off
    "aug_contrast": 0.0,            # ... a contrast factor (blend with the image's mean gray value)
    "aug_saturation": 0.0,          # ... a saturation factor (blend with the pixel's gray value)
    "aug_flip": 0.0,                # in [0, 1]: probability that a training image (one image slot in grouped batches) is mirrored left-right; its boxes are mirrored and the left / right words of its queries swapped (dat_loader.swap_left_right); 0 = off
    "aug_expand_max": 1.0,          # > 1 (in [1, 4]): zoom-out — the image is placed on a canvas of r ~ U(1, aug_expand_max) times its sides before the window is drawn (dat_loader.draw_augment_geom); 1 = off
    "aug_fill": [124, 116, 104],    # ... the canvas colour, RGB integers 0..255 (the ImageNet mean); also the colour a warp (aug_rotate / aug_shear) brings in from outside the image
    "aug_rotate": 0.0,              # > 0 (degrees, in [0, 30]): the resized training image is rotated about its centre by theta ~ U(-v, v) (dat_loader.warp_matrix, augment_host step 6; zsg_augment_warp_u8_batched with gpu_img_resize); the box becomes the clipped bounding box of its warped corners (dat_loader.warp_box); 0 = off
    "aug_shear": 0.0,               # > 0 (degrees, in [0, 20]): ... and sheared along x by phi ~ U(-v, v), one warp M = R(theta) S(phi); 0 = off
    "aug_warp_keep": 0.8,           # in (0, 1]: a drawn (theta, phi) is used only when every box of the item (of the image slot in grouped batches) keeps this fraction of its warped bounding box inside the image; else both are halved, at most four times, then the warp is dropped (dat_loader.settle_warp)
    "aug_blur": 0.0,                # 0, or in [0.1, 2.5]: Gaussian blur of the training image with sigma ~ U(0.1, v) output pixels, radius min(8, ceil(3 sigma)) (dat_loader.blur_taps, augment_host step 7); 0 = off
    "aug_blur_p": 0.5,              # ... applied when a uniform draw is below this probability (in [0, 1])
    "box_iou_loss": "none",         # "giou" / "diou": ZSGLoss adds lamb_iou * (that IoU loss of the decoded positive boxes) to the criterion and reports it as iou_ls (zsg_loss_fwd_bwd_iou); "none" = off
    "lamb_iou": 1.0,                # ... its weight (>= 0); lamb_reg = 0 with it trains on the IoU term alone
    "cls_quality": "none",          # "qfl" / "vfl": the att logit is trained towards the IoU of the anchor's decoded box with the annotation (Quality Focal / Varifocal loss, zsg_loss_fwd_bwd_q) and ZSGLoss also reports pos_iou; needs use_focal, no use_softmax, gamma >= 1; "none" = the reference's focal term
    "matcher": "iou",               # which anchors are positive: "iou" = the reference's fixed rule (IoU > matching_threshold, or the arg-max anchor); "atss" = Adaptive Training Sample Selection on the device (zsg_match_atss + zsg_loss_fwd_bwd_m): per pyramid level the atss_topk anchors nearest the annotation's centre, of those the ones with IoU >= mean + std whose centre lies inside the annotation, and the arg-max anchor; needs use_multi, no use_softmax; matching_threshold is not read; "tal" = task-aligned assignment from the network's own predictions (tal_topk / tal_alpha / tal_beta below)
    "eval_dtype": "fp32",           # "bf16": the convolutions of the EVAL forward (validation, only_val / only_test, Evaluator.predict, the many-phrases plan) run on bf16 MFMA with fp32 accumulation (zsg_conv_igemm_bf16; ZSGNet.eval_precision) — activations stay fp32 in memory, the stem, the LSTM and the language map stay fp32, training is untouched; "bf16_act": "bf16", and the activations between the stem's max-pool and the heads' last convolution are stored as bf16 (half the activation bytes of an eval plan; rounded once where stored, arithmetic in fp32; the outputs stay fp32); "fp32" = every plan as before
    "eval_tta": "none",             # "flip": every EVAL forward (validation, only_val / only_test, EMA validation, Evaluator.predict, the many-phrases plan) also runs the batch mirrored left-right — the image mirrored on the GPU, the left / right words of the query swapped by the loader (`qvec_flip`, dat_loader.swap_left_right) — as rows B..2B-1 of ONE eval forward of 2B rows, and the two predictions are averaged per anchor in regression-parameter space (tx changes sign; zsg_tta_flip_stage_* / zsg_tta_flip_merge; ZSGNet.eval_tta); the output keeps its [B, A, 5] shape; training is untouched; "none" = every plan as before
    "eval_scales": [],              # e.g. [0.75, 1.25]: multi-scale test-time augmentation — every EVAL forward also runs the batch resampled on the GPU (Pillow bicubic of the batch's own H x W pixels, zsg_resize_u8_batched) to (round(s H), round(s W)) for every entry s, each pass the plain eval plan of its geometry (with its own mirrored rows under eval_tta = "flip"); the output dict is pass 0's plus `tta_att_bbx_out` [B, sum A_s, 5] and `tta_feat_sizes`, which the evaluator scores over the concatenated anchor tables (arg-max / top-k NMS over all scales; ZSGNet.eval_scales); at most 4 entries in [0.5, 2], none rounding to the base size or to another entry's; needs the uint8 batch of gpu_img_normalise; training is untouched; [] = every plan as before
    "eval_box_vote": 0.0,           # in (0, 1]: in eval mode the evaluator replaces every kept box (eval_topk rows, K = 1 included) by the score-weighted mean of the eval_pre_nms candidates whose IoU with it is >= this (zsg_eval_vote, tests/vote_ref.py): Acc / Acc@K / pred_boxes / topk_boxes are the voted boxes', pred_boxes_raw keeps the arg-max box; scores, order and count stay; 0 = off
    "eval_nms": "hard",             # how the evaluator picks the eval_topk rows (and the rows eval_box_vote refines): "hard" = greedy NMS at eval_nms_thr (zsg_eval_topk); "soft_linear" / "soft_gauss" = Soft-NMS (Bodla et al. 2017; zsg_eval_topk_soft, tests/softnms_ref.py): a picked box multiplies the score of every other candidate by 1 - IoU where IoU > eval_nms_thr (linear) or by exp(-IoU^2 / eval_soft_sigma) (gauss), selection goes on over the decayed scores, topk_scores are the decayed scores; row 0 stays the arg-max box
    "eval_soft_sigma": 0.5,         # ... the Gaussian decay's sigma (> 0, finite); read by "soft_gauss" only
    "eval_soft_min_score": 0.001,   # ... the score floor of both soft rules, in [0, 1): the rows end at the first decayed score below it (topk_n < K)
    "wgrad_dtype": "fp32",          # "bf16": the convolution weight gradients of the TRAINING backward run on bf16 MFMA with fp32 accumulation (zsg_conv_wgrad_bf16; ZSGNet.wgrad_precision) — src, dy and the gradients stay fp32 in memory, the forward, the data gradients, the stem and the small directly lowered weight gradients stay fp32
    "train_dtype": "fp32",          # "bf16_head": in TRAINING plans the forward convolutions and the data gradients of the pyramid (backbone.fpn.*) and the head stacks run on bf16 MFMA with fp32 accumulation (zsg_conv_igemm_bf16 / zsg_conv_igemm_bf16_m; ZSGNet.train_precision) — activations, weights and gradients stay fp32 in memory; the encoder, every BatchNorm-fused launch, the query encoder and the weight gradients (wgrad_dtype) are untouched
    "enc_dtype": "fp32",            # "bf16_fwd": in TRAINING plans the forward convolutions of a ResNet encoder behind the stem (backbone.encoder.*) run on bf16 MFMA with fp32 accumulation and the fused BatchNorm statistics (zsg_conv_igemm_bf16_bn; ZSGNet.encoder_precision) — activations, weights and gradients stay fp32 in memory; the stem, the convolutions that apply a pending BatchNorm in their loader, the whole backward (fp32 data gradients, weight gradients as wgrad_dtype says) and the SSD-VGG encoder are untouched
    "enc_bwd_dtype": "fp32",        # "bf16": in TRAINING plans the data gradients of a ResNet encoder behind the stem (backbone.encoder.*) run on bf16 MFMA with fp32 accumulation (zsg_conv_igemm_bf16_m; where one completes a BatchNorm's dout, zsg_conv_igemm_bf16_bnb with that BatchNorm's backward sums in its epilogue; ZSGNet.encoder_backward_precision) — activations, weights and gradients stay fp32 in memory; the forward, the stem, the pyramid's data gradients into C3-C5, the weight gradients (wgrad_dtype) and the SSD-VGG encoder are untouched; independent of enc_dtype
    "atss_topk": 9,                # ... candidates per pyramid level (1 .. 16)
    "tal_topk": 13,                # matcher "tal" (task-aligned assignment, zsg_match_tal + zsg_loss_fwd_bwd_m): per annotation the tal_topk (1 .. 32) anchors with the largest sigmoid(att)^tal_alpha * IoU(decoded box, annotation)^tal_beta among those whose centre lies inside the annotation, and the arg-max anchor; reads the network's output, no gradient through the selection; needs use_multi, no use_softmax; matching_threshold and atss_topk are not read
    "tal_alpha": 1.0,              # ... the exponent of the score (>= 0, finite)
    "tal_beta": 6.0,               # ... the exponent of the IoU (>= 0, finite); 13 / 1 / 6 are TOOD's published values, not tuned here
    # configs/ds_info.json: where each dataset's images and csv files live (override with --ds_info.<name>.<key>=...)
    "ds_info": {name: {"data_dir": f"./data/{root}", "img_dir": f"./data/{imgs}",
                       **{f"{s}_csv_file": f"./data/{csv}/csv_dir/{f}.csv" for s, f in (("trn", trn), ("val", "val"), ("test", "test"))}}
                for name, root, imgs, csv, trn in (
                    ("flickr30k", "flickr30k", "flickr30k/flickr30k_images", "flickr30k", "train_flat"),
                    ("refclef", "referit/refclef", "referit/saiapr_tc12_images", "referit", "train_flat"),
                    ("flickr30k_c0", "flickr30k", "flickr30k/flickr30k_images", "flickr30k_c0", "train"),
                    ("flickr30k_c1", "flickr30k", "flickr30k/flickr30k_images", "flickr30k_c1", "train"),
                    ("vg_split_c2", "visual_genome/vg_split", "visual_genome", "vg_split_c2", "train"),
                    ("vg_split_c3", "visual_genome/vg_split", "visual_genome", "vg_split_c3", "train"))},
}


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        if self.get("_frozen", False) and k != "_frozen":
            raise AttributeError("cfg is frozen")
        self[k] = v

    def freeze(self):
        dict.__setitem__(self, "_frozen", True)

    def clone(self) -> "Cfg":
        c = Cfg(copy.deepcopy({k: v for k, v in self.items() if k != "_frozen"}))
        return c


def get_cfg(**overrides) -> Cfg:
    cfg = Cfg(copy.deepcopy(DEFAULTS))
    return update_from_dict(cfg, overrides)


def _decode(v):
    if isinstance(v, str):
        try:
            return ast.literal_eval(v)
        except (ValueError, SyntaxError):
            return v
    return v


def update_from_dict(cfg: Cfg, dct: Dict[str, Any], key_maps: Dict[str, str] = None) -> Cfg:
    """extended_config.py:46-90: every key must already exist and keep its type."""
    for full_key, v in dct.items():
        d = cfg
        parts = full_key.split(".")
        for sub in parts[:-1]:
            assert sub in d, f"key {full_key} doesnot exist"
            d = d[sub]
        sub = parts[-1]
        assert sub in d, f"key {full_key} doesnot exist"
        old = d[sub]
        val = v if isinstance(old, str) else _decode(v)
        if isinstance(old, float) and isinstance(val, int) and not isinstance(val, bool):
            val = float(val)
        assert isinstance(val, type(old)), f"key {full_key}: expected {type(old).__name__}, got {type(val).__name__}"
        d[sub] = val
    return cfg


def ratios_scales(cfg):
    """main_dist.py:24-31: ratios / scales are strings in the json and are eval'd."""
    import numpy as np
    ratios = eval(cfg["ratios"], {}) if not isinstance(cfg["ratios"], list) else cfg["ratios"]
    sc = eval(cfg["scales"], {}) if not isinstance(cfg["scales"], list) else cfg["scales"]
    return ratios, cfg["scale_factor"] * np.array(sc)

"""Adapt the class head of a pretrained model to a new charset, on the device.

  finetuning.py --new_class_embedding (+ engine.train_one_epoch_CTC)   ->   new_class_head / smart_mapping_init + HeadTrainer
  `python -m dtlr_amd.adapt`                                           ->   a checkpoint that
                                                                            evaluation.load_model(new_class_embedding=True,
                                                                            fix_enc_out_class=True) loads

The reference adapts a model to a new script by rebuilding the class heads for the new charset (finetuning.py:422-539) and training
them against the CTC loss (engine.py:160-260).  That loop calls `criterion.loss_CTC(outputs, targets, None, None)` (engine.py:200): the
CTC loss on the FINAL pred_logits only, and with --new_class_embedding the optimizer holds only the class heads.  With
dec_pred_class_embed_share (every shipped config) pred_logits = class_embed(hs[-1]) is one shared Linear; the decoder's own copy and the
two-stage head receive no gradient from this loss (the top-k is not differentiable, the reference points are detached) and AdamW skips
parameters without a gradient.  dropout = 0, use_dn = False and FrozenBN make the training-mode forward equal the eval forward.  So one
step is: the frozen forward this package already has, the CTC loss's gradient with respect to the logits
(dtlr_ctc_loss_interleaved_backward), dW = dlogits^T hs (dtlr_head_grad), clip (dtlr_grad_norm_scale), AdamW (dtlr_adamw_step) -- four
HIP entry points, no backward through the trunk.  Nothing in a step waits for the device: the host's part is packing the label lists
into the targets tensor and its (pageable) copy to the device; the loss stays a device tensor until the caller reads it.

With the detection criterion (--loss set | ctc+set) the same trainer also trains the shared box head `bbox_embed` and takes the losses of
every decoder output (--train class,box, --aux-loss): still no backward through the trunk, whose states are
constants of both heads' gradients (dtlr_box_refine_grad, dtlr_box_mlp_grad).

--train ..,tail also trains the decoder's tail: linear1, linear2 and norm3 of the last decoder layer and
transformer.decoder.norm, everything the loss reaches without crossing an attention.  Its gradient starts from the last layer's state after
norm1, a constant of the frozen trunk (dtlr_head_dx, dtlr_box_mlp_dx, dtlr_ln_backward, dtlr_ffn_recompute, dtlr_ffn_grad).

--train ..,tail,cross goes one block deeper: the last decoder layer's deformable cross-attention -- its sampling_offsets,
attention_weights and output_proj -- and the norm1 after it, the parameters that place a query on a character.  Everything below the block
(the state after norm2, the query position embedding, the reference points, the value map) is a constant of the frozen trunk, and of the
deformable attention's backward only the two gathers are needed (dtlr_cross_recompute, dtlr_msda_query_grad, dtlr_cross_dow).

--train ..,tail,cross,self trains the last decoder layer whole: its self-attention -- in_proj, out_proj -- and the norm2
after it, where the character queries of a line talk to each other.  The layer's input state and the query position embedding are the
constants of the frozen trunk; everything from there up is recomputed in fp32 from the masters (dtlr_self_recompute), the cross block then
starts from THAT state after norm2, and the attention core's backward is dtlr_mha_grad.

--augment default | full trains on the reference's augmented lines: make_coco_transforms("train")'s random erasing
(and, with --aug-scales, its random resize per line) drawn on the host from (seed, epoch, line) and applied by the launch that resizes
the line (dtlr_augment_lines).  --resident decodes every file once into one device buffer (transforms.DeviceLineSet) and feeds every step
from it; --val-labels / --val-mode run the held-out, never augmented lines through the forward after every epoch and print val loss_CTC
and val CER.  Without these flags the loop runs the launches it ran.

--synth-fonts A.ttf,B.ttf | builtin (or --synth-atlas atlas.npz) with --synth-lines N trains on synthetic lines rendered on the device
(dtlr_amd/synthlines.py, dtlr_synth_lines): no --images / --labels, every character carries the box its layout
gave it (--loss set / ctc+set take them without --boxes), and the start of every epoch renders fresh lines into the same resident
pool.  --augment, --batching, --val-* (real held-out lines) and every --train group work as on a resident set.  Without these flags the
loop runs the launches it ran.
"""
from __future__ import annotations

import argparse
import sys
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import evaluation as E
from . import ops


def smart_mapping_init(old_head, old_charset: Sequence, new_charset: Sequence, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """--smart_mapping (finetuning.py:454-510): the rows of the new head are rows of the old one.  A character present in both charsets
    takes its own old row (first occurrence in old_charset); the other new characters take the old rows no shared character uses, in a
    seeded random order.  When there are fewer unused rows than new characters, the list is first topped up with seeded random rows, as
    the reference does.  old_head: an nn.Linear or a (weight [C_old, D], bias [C_old]) pair.  Returns (weight [C_new, D], bias [C_new]).

    NOT the reference's random stream: it draws from the unseeded global np.random; here the draws come from
    np.random.Generator(PCG64(seed)), so the same inputs always give the same head."""
    w, b = (old_head.weight, old_head.bias) if isinstance(old_head, nn.Linear) else old_head
    w, b = w.detach(), b.detach()
    old_charset, new_charset = list(old_charset), list(new_charset)
    if w.shape[0] != len(old_charset):
        raise ValueError(f"smart_mapping_init: the old head has {w.shape[0]} rows, old_charset {len(old_charset)} characters")
    mapping = smart_mapping(old_charset, new_charset, seed)
    idx = torch.as_tensor(mapping, dtype=torch.long, device=w.device)
    return w[idx].clone(), b[idx].clone()


def smart_mapping(old_charset: Sequence, new_charset: Sequence, seed: int = 0) -> List[int]:
    """new class index -> old class index of smart_mapping_init."""
    old_charset, new_charset = list(old_charset), list(new_charset)
    first = {}
    for i, ch in enumerate(old_charset):
        first.setdefault(ch, i)
    mapping: Dict[int, int] = {}
    unused = list(range(len(old_charset)))
    not_mapped = []
    for i, ch in enumerate(new_charset):
        if ch in first:
            mapping[i] = first[ch]
            if mapping[i] in unused:                      # a character listed twice in new_charset shares its old row
                unused.remove(mapping[i])
        else:
            not_mapped.append(i)
    g = np.random.Generator(np.random.PCG64(seed))
    while len(unused) < len(not_mapped):
        unused.append(int(g.integers(0, len(old_charset))))
    unused = [unused[k] for k in g.permutation(len(unused))]
    for k, i in enumerate(not_mapped):
        mapping[i] = unused[k]
    return [mapping[i] for i in range(len(new_charset))]


def new_class_head(model, num_classes: int, weight: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None):
    """The head rebuild of finetuning.py:422-452,524-529 on `model` (a dtlr_amd DINO): one fresh Linear(hidden -> num_classes) shared by
    the decoder layers under `class_embed`, a separate bare Linear under `transformer.decoder.class_embed` (the reference creates it;
    no forward uses it), `enc_out_class_embed` KEPT (the non-smart branch, :364-366 / :524-529).  weight / bias: the initial head
    (smart_mapping_init's result); default: nn.Linear's own initialisation, as in the reference.  The resulting state dict is what
    evaluation.load_model(new_class_embedding=True, fix_enc_out_class=True, charset_size=num_classes) loads."""
    if not model.dec_pred_class_embed_share:
        raise NotImplementedError("new_class_head: written for dec_pred_class_embed_share (every shipped config)")
    old = model.class_embed[0]
    d, dev = old.weight.shape[1], old.weight.device
    head = nn.Linear(d, int(num_classes))
    if weight is not None:
        with torch.no_grad():
            head.weight.copy_(weight)
            head.bias.copy_(bias)
    model.class_embed = nn.ModuleList([head for _ in range(model.transformer.num_decoder_layers)]).to(dev)
    model.transformer.decoder.class_embed = nn.Linear(d, int(num_classes)).to(dev)
    model._engine = None
    model.eval()
    return model


TRAINABLE = ("class", "box", "tail", "cross")        # the groups up to DESIGN.md section 23, in the flat buffer's order
TRAINABLE_ALL = TRAINABLE + ("self",)                # the groups up to DESIGN.md section 24
TRAINABLE_FULL = TRAINABLE_ALL + ("value",)          # what HeadTrainer(train=..) and --train may name, in the flat buffer's order


@dataclass
class ParamGroup:
    """One trained group of HeadTrainer's flat buffer: the model's parameters in flat order, their shapes, where the group lies in the
    buffer, its state-dict keys (values, exp_avg, exp_avg_sq) and how its master views are handed to the engine."""
    params: List[torch.Tensor]
    shapes: List[Tuple[int, ...]]
    offset: int
    n: int
    keys: Tuple[str, str, str]
    attach: Callable

    def of(self, flat: torch.Tensor) -> torch.Tensor:
        """the group's slice of a flat buffer (param, a moment or grad)"""
        return flat[self.offset: self.offset + self.n]

    def views(self, flat: torch.Tensor) -> List[torch.Tensor]:
        """the group's tensors as views of a flat buffer, in flat order"""
        out, o = [], self.offset
        for shape in self.shapes:
            k = int(np.prod(shape))
            out.append(flat[o:o + k].view(shape))
            o += k
        return out


def _model_params(model, name: str) -> List[torch.Tensor]:
    """group name -> the model's parameters in the flat order: the shared class head [W, b]; the shared box MLP [W0, b0, W1, b1, W2,
    b2]; the tail (ops.TAIL_NAMES): linear1, linear2 and norm3 of the last decoder layer, then transformer.decoder.norm; the cross block
    (ops.CROSS_NAMES): sampling_offsets, attention_weights and output_proj of the last decoder layer's cross_attn, then its norm1; the self
    block (ops.SELF_NAMES): in_proj and out_proj of the last decoder layer's self_attn, then its norm2; "value": the weight and bias of
    the last decoder layer's cross_attn.value_proj"""
    if name == "class":
        return [model.class_embed[0].weight, model.class_embed[0].bias]
    if name == "box":
        return [p for l in model.bbox_embed[0].layers for p in (l.weight, l.bias)]
    dec = model.transformer.decoder
    last = dec.layers[len(dec.layers) - 1]
    if name == "value":
        return [last.cross_attn.value_proj.weight, last.cross_attn.value_proj.bias]
    if name == "self":
        a = last.self_attn
        return [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, last.norm2.weight, last.norm2.bias]
    if name == "cross":
        a = last.cross_attn
        return [a.sampling_offsets.weight, a.sampling_offsets.bias, a.attention_weights.weight, a.attention_weights.bias, a.output_proj.weight,
                a.output_proj.bias, last.norm1.weight, last.norm1.bias]
    return [last.linear1.weight, last.linear1.bias, last.linear2.weight, last.linear2.bias, last.norm3.weight, last.norm3.bias,
            dec.norm.weight, dec.norm.bias]


# group name -> (its state-dict keys, how its master views reach the engine)
_GROUPS = {"class": (("head", "exp_avg", "exp_avg_sq"), lambda eng, v: eng.set_class_head(v[0], v[1])),
           "box": (("box_head", "box_exp_avg", "box_exp_avg_sq"), lambda eng, v: eng.set_box_head(v[0::2], v[1::2])),
           "tail": (("tail", "tail_exp_avg", "tail_exp_avg_sq"), lambda eng, v: eng.set_decoder_tail(v[0:2], v[2:4], v[4:6], v[6:8])),
           "cross": (("cross", "cross_exp_avg", "cross_exp_avg_sq"), lambda eng, v: eng.set_decoder_cross(v[0:2], v[2:4], v[4:6], v[6:8])),
           "self": (("self", "self_exp_avg", "self_exp_avg_sq"), lambda eng, v: eng.set_decoder_self(v[0], v[1], v[2:4], v[4:6])),
           "value": (("value", "value_exp_avg", "value_exp_avg_sq"), lambda eng, v: eng.set_decoder_value(v))}


def _cat(ts):
    """torch.cat, without the copy when there is one tensor (the step over one output)"""
    return ts[0] if len(ts) == 1 else torch.cat(ts)


class HeadTrainer:
    """Trains `model.class_embed` (the Linear shared by the decoder layers) against the CTC loss with AdamW, everything on the device.

    The fp32 master copy of the head lives in one flat buffer (W row-major, then b) beside its AdamW moments; before every forward it is
    handed to the engine (DTLREngine.set_class_head), so the logits always come from the engine's own class-head path -- the 16-bit
    engines' hi + lo products, the f32s engine's split products -- on the current master weights.  The trunk is frozen: `cache` returns
    the decoder states and boxes of a batch, and `step_cached` trains on them without running the trunk again.

    Defaults are the reference's (config/Latin_CTC.py:5,14,18: lr 1e-5, weight_decay 1e-4, clip_max_norm 0.01; AdamW's own betas / eps).

    Two deviations from the reference's loop (engine.train_one_epoch_CTC):
      * the clip norm is taken over the head's gradient only.  The reference clips over model.parameters() (engine.py:213-214), trunk
        included, which needs a full backward that this package does not have;
      * `enc_out_class_embed` is kept as it is (finetuning.py:364-366 / 524-529, the non-smart branch): the two-stage selection keeps
        scoring with the pretrained head.
    `transformer.decoder.class_embed` and `enc_out_class_embed` get no gradient from this loss in the reference either, and AdamW skips
    parameters without one (no weight decay on them), so leaving them alone is not a deviation.

    step / step_cached return {"loss_CTC": 0-d fp32 CUDA tensor} -- the loss BEFORE the update, as the reference logs it; reading it is
    the caller's (only) host synchronisation.  max_norm None or <= 0: no clipping.

    loss: "ctc" (default: the above, unchanged), "set" or "ctc+set".  The set modes train against the reference's detection criterion
    (dtlr_amd/criterion.py: Hungarian matching of the main output against the line's character boxes, then the sigmoid focal loss):
    step / step_cached take `target_boxes` (per line [T,4] cxcywh in 0..1, one box a label) as well, the head's dlogits is
    CTC_loss_coef dCTC + cls_loss_coef dfocal (the coefficients of config/Latin_CTC.py:77,81, both 1), the matcher's costs are the
    reference's (set_cost_class 2, set_cost_bbox 5, set_cost_giou 2, focal_alpha 0.25), and the returned dict also carries loss_ce,
    loss_bbox, loss_giou, cardinality_error and class_error of the main output.  The matcher reads the solver's status: one host
    synchronisation a step.  A third deviation, in the set modes only:
      * by default the focal loss is taken on the main output only.  The reference also sums the auxiliary layers' and the intermediate
        output's loss_ce, which reach the shared head too: aux_loss=True adds the auxiliary layers (not the intermediate output, whose
        heads are the two-stage ones).

    train: a subset of {"class", "box"} (default: the class head alone, the above unchanged in bits).  "box" also trains the shared box
    head `bbox_embed` against bbox_loss_coef x L1 + giou_loss_coef x GIoU of the matched pairs (5 and 2,
    config/Latin_CTC.py:79-80), exactly and with the trunk frozen: every use of the box head's output inside the trunk is detached in
    the reference, so the decoder states are constants of this gradient too; "look forward twice" makes an output's box depend on the MLP
    at two layers' states, both are followed (ops.box_refine_grad, ops.box_mlp_grad).  It needs a set loss (the CTC loss has no gradient
    for boxes) and the full forward every step (the forward depends on the box head: no cache / step_cached).
    aux_loss=True: every decoder output is matched and weighted as the reference weighs it (the same coefficients for every layer); False:
    only the main output's row of weights is non-zero -- its box gradient still reaches the state one layer below.  With either, the
    matcher runs on all decoder outputs in one launch, the trained parameters, their moments and their gradient share ONE flat buffer
    ([class W | class b | box W0 | b0 | W1 | b1 | W2 | b2]), the clip norm is taken over all of it (closer to the reference's global
    clip than the head's own) and one AdamW launch updates it.  The returned dict also carries loss_ce_<l>, loss_bbox_<l>,
    loss_giou_<l> of auxiliary output l, and `last_states` keeps the step's hs_all, tgt_all, refs, stacked outputs and match_q.

    train may also name "tail" (DESIGN.md section 22): linear1, linear2 and norm3 of the LAST decoder layer and transformer.decoder.norm,
    1,051,904 parameters at dim_feedforward 2048 -- everything after the last cross-attention, which the loss reaches without a backward
    through an attention.  The flat buffer grows to [class | box | W1 | b1 | W2 | b2 | norm3.w | norm3.b | dec_norm.w | dec_norm.b], still
    under one clip norm and one AdamW launch with uniform decay.  It works with every loss ("ctc" reaches the tail through dlogits alone)
    and with or without aux_loss (decoder.norm's affine parameters then take gradient from every output).  With a set loss the box terms
    are weighted with bbox_loss_coef / giou_loss_coef whether or not "box" is trained: the tail moves pred_boxes through the decoder
    states, and likewise the class terms whether or not "class" is.  The gradient is the fp32 function's at the engine's states: the
    last layer's state after norm1 and the lower layers' outputs are the engine's, the FFN's output and norm3's are recomputed in fp32
    from the master weights.  With "tail" and neither "box" nor aux_loss, `cache` returns (the last layer's FFN input, its reference
    points) and `step_cached` runs DTLREngine.tail_forward on them: the same step without the trunk.

    train may also name "cross" (DESIGN.md section 23), with "tail": sampling_offsets, attention_weights and output_proj of the LAST decoder
    layer's cross-attention and the norm1 after it, 164,992 parameters -- where a query looks.  The flat buffer grows by [so.W | so.b | aw.W |
    aw.b | out.W | out.b | norm1.w | norm1.b], under the same clip norm and AdamW launch.  It needs "tail" (the gradient passes through the
    FFN chain either way), works with every loss and with or without aux_loss (the auxiliary outputs do not depend on the last layer), and
    needs the full forward every step: the cache would have to hold the batch's value map (no cache / step_cached).  The block's inputs
    -- the state after norm2, the query position embedding, the reference points, the value map -- are the engine's (forward's
    return_hidden="cross"); everything from there up is recomputed in fp32 from the masters (ops.cross_recompute), and the tail's chain then
    starts from THIS recomputed state after norm1, not from the engine's.  Of the deformable attention's backward only the gradients with
    respect to the sampling locations and the attention weights are taken (ops.msda_query_grad); the one with respect to the value map
    leads to frozen parameters only.

    train may also name "self" (DESIGN.md section 24), with "cross" (and so "tail"): in_proj and out_proj of the LAST decoder layer's
    self-attention and the norm2 after it, 263,680 parameters -- the last decoder layer is then trained whole, and layers 0 .. L-2, the encoder
    and the backbone are the constants.  The flat buffer grows by [in_proj.W | in_proj.b | out_proj.W | out_proj.b | norm2.w | norm2.b] at its
    end, under the same clip norm and AdamW launch.  The block's inputs -- the layer's input state and the query position embedding -- are the
    engine's (forward's return_hidden="self"); everything from there up is recomputed in fp32 from the masters (ops.self_recompute), the cross
    block's chain starts from THIS recomputed state after norm2 and hands back the gradient at it (ops.cross_grad's return_ds), and the
    attention core's backward is ops.mha_grad.  The terms that land on the layer's input are dropped.  No cache / step_cached.

    train may also name "value" (DESIGN.md section 25), with "self" (and so "cross" and "tail"): the weight and bias of the LAST decoder
    layer's cross_attn.value_proj, 65,792 parameters -- with it every parameter of the last decoder layer is trained.  The flat buffer grows by
    [value_proj.W | value_proj.b] at its end, under the same clip norm and AdamW launch.  Its inputs -- the decoder's memory and the flat
    padding mask -- are the engine's (forward's return_hidden="value"); the layer's value map is recomputed in fp32 from the master
    (memory Wv^T + bv, the rows under the mask zero), the cross block samples THAT map, hands back the gradient at the sampler's output
    (ops.cross_grad's return_do), ops.msda_value_grad turns it into the gradient at the map, and the weight gradient is ops.head_grad of it
    against memory.  The term that lands on memory is dropped.  No cache / step_cached.

    How it is laid out.  `self.groups` maps each trained group ("class", "box", "tail", "cross", "self", "value", in this order) to its ParamGroup: the model's
    parameters in flat order, their shapes, the group's offset and length in the flat buffers (param, exp_avg, exp_avg_sq, grad), its
    state-dict keys and the engine setter it is handed to.  weight / bias / box_head() / tail() / cross() / self_block(), _engine(), the step's gradient slices,
    state_dict / load_state_dict and write_back read that table and nothing else knows an offset.  There is ONE step routine, `_update`,
    over the L decoder outputs it is given: every output of return_hidden="all" / "tail", or -- the class head on the main output, and
    every cached step -- the one-output dict `_main_output` builds (L = 1: no loss_*_<l> keys, nothing stacked or concatenated, the
    four operators of the module docstring with the same arguments).  `last_states` is therefore filled after every step, the default
    one included (hs_all = [hs], tgt_all = [None], refs = [None] or the cached reference points)."""

    def __init__(self, model, lr: float = 1e-5, weight_decay: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_norm: Optional[float] = 0.01, loss: str = "ctc", CTC_loss_coef: float = 1.0, cls_loss_coef: float = 1.0,
                 train: Sequence[str] = ("class",), aux_loss: bool = False, bbox_loss_coef: float = 5.0, giou_loss_coef: float = 2.0):
        train = (train,) if isinstance(train, str) else tuple(train)
        if not train or set(train) - set(TRAINABLE_FULL):
            raise ValueError(f"HeadTrainer: train {train!r} is not a non-empty subset of {TRAINABLE_FULL!r}")
        if loss not in ("ctc", "set", "ctc+set"):
            raise ValueError(f"HeadTrainer: loss {loss!r} is not one of ctc, set, ctc+set")
        if "box" in train and loss == "ctc":
            raise ValueError("HeadTrainer(train=('box', ..)): the CTC loss has no gradient for boxes -- loss must be 'set' or 'ctc+set'")
        if aux_loss and loss == "ctc":
            raise ValueError("HeadTrainer(aux_loss=True): the CTC loss is taken on the main output only -- loss must be 'set' or 'ctc+set'")
        if "cross" in train and "tail" not in train:
            raise ValueError("HeadTrainer(train=('cross', ..)): 'cross' requires 'tail' -- the gradient of the cross-attention block passes "
                             "through the last FFN and the norms either way")
        if "self" in train and "cross" not in train:
            raise ValueError("HeadTrainer(train=('self', ..)): 'self' requires 'cross' -- the gradient of the self-attention block passes "
                             "through the cross-attention block and the tail either way")
        if "value" in train and "self" not in train:
            raise ValueError("HeadTrainer(train=('value', ..)): 'value' requires 'self' -- the gradient of the value projection passes through "
                             "the cross-attention block, which then starts from the recomputed state of the self-attention block")
        if "box" in train and (getattr(model.cfg, "use_detached_boxes_dec_out", False) or not model.dec_pred_bbox_embed_share):
            raise NotImplementedError("HeadTrainer(train=('box', ..)): written for the shared box head with look-forward-twice "
                                      "(dec_pred_bbox_embed_share, use_detached_boxes_dec_out = False: every shipped config)")
        self.train = tuple(k for k in TRAINABLE_FULL if k in train)
        self.aux_loss = bool(aux_loss)
        self.bbox_loss_coef, self.giou_loss_coef = float(bbox_loss_coef), float(giou_loss_coef)
        self.every_output = "box" in self.train or "tail" in self.train or self.aux_loss          # the step reads every decoder layer's states
        if not model.dec_pred_class_embed_share:
            raise NotImplementedError("HeadTrainer: written for dec_pred_class_embed_share (every shipped config)")
        head = model.class_embed[0]
        if model.training:
            raise RuntimeError("HeadTrainer: call model.eval() -- the frozen trunk runs its inference forward")
        self.model = model
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps)
        self.max_norm = float(max_norm) if max_norm is not None else 0.0
        self.loss, self.CTC_loss_coef, self.cls_loss_coef = loss, float(CTC_loss_coef), float(cls_loss_coef)
        self.matcher = None
        if loss != "ctc":
            from .criterion import HungarianMatcher
            self.matcher = HungarianMatcher(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0, focal_alpha=0.25)
        self.C, self.D = int(head.weight.shape[0]), int(head.weight.shape[1])
        self.F = 0
        if "tail" in self.train:
            layers = model.transformer.decoder.layers
            last = layers[len(layers) - 1]
            if getattr(model.cfg, "transformer_activation", "relu") != "relu" or getattr(model.cfg, "dropout", 0.0) != 0.0:
                raise NotImplementedError("HeadTrainer(train=('tail', ..)): written for the ReLU FFN without dropout (every shipped config)")
            if any(o is last or o.linear1.weight is last.linear1.weight or o.linear2.weight is last.linear2.weight or o.norm3.weight is last.norm3.weight
                   for o in list(layers)[:-1]):
                raise NotImplementedError("HeadTrainer(train=('tail', ..)): the decoder layers share parameters -- the last layer's FFN is then "
                                          "not the tail alone")
            self.F = int(last.linear1.weight.shape[0])
        if "cross" in self.train:
            layers = model.transformer.decoder.layers
            last = layers[len(layers) - 1]
            if any(o.cross_attn is last.cross_attn or o.cross_attn.output_proj.weight is last.cross_attn.output_proj.weight or o.norm1.weight is last.norm1.weight
                   for o in list(layers)[:-1]):
                raise NotImplementedError("HeadTrainer(train=('cross', ..)): the decoder layers share parameters -- the last layer's cross-attention is "
                                          "then not the block alone")
            geometry = tuple(getattr(model.cfg, k, None) for k in ("dec_n_points", "nheads", "num_feature_levels"))
            if geometry != (4, 8, 4):
                raise NotImplementedError(f"HeadTrainer(train=('cross', ..)): written for dec_n_points 4, nheads 8, num_feature_levels 4 (every "
                                          f"shipped config), not {geometry}")
        if "self" in self.train:
            layers = model.transformer.decoder.layers
            last = layers[len(layers) - 1]
            if getattr(model.cfg, "transformer_activation", "relu") != "relu" or getattr(model.cfg, "dropout", 0.0) != 0.0:
                raise NotImplementedError("HeadTrainer(train=('self', ..)): written for the ReLU FFN without dropout (every shipped config)")
            if any(o.self_attn is last.self_attn or o.self_attn.in_proj_weight is last.self_attn.in_proj_weight
                   or o.self_attn.out_proj.weight is last.self_attn.out_proj.weight or o.norm2.weight is last.norm2.weight for o in list(layers)[:-1]):
                raise NotImplementedError("HeadTrainer(train=('self', ..)): the decoder layers share parameters -- the last layer's self-attention is "
                                          "then not the block alone")
            geometry = (getattr(model.cfg, "nheads", None), getattr(model.cfg, "hidden_dim", None))
            if geometry != (8, 256):
                raise NotImplementedError(f"HeadTrainer(train=('self', ..)): written for nheads 8 x 32 channels (hidden_dim 256: every shipped config), "
                                          f"not nheads, hidden_dim = {geometry}")
        if "value" in self.train:
            layers = model.transformer.decoder.layers
            last = layers[len(layers) - 1]
            if any(o.cross_attn is last.cross_attn or o.cross_attn.value_proj.weight is last.cross_attn.value_proj.weight for o in list(layers)[:-1]):
                raise NotImplementedError("HeadTrainer(train=('value', ..)): the decoder layers share parameters -- the last layer's value projection "
                                          "is then not the block alone")
        # the ONE table of what is trained: every slice of param / exp_avg / exp_avg_sq / grad below is a lookup in it
        self.groups: Dict[str, ParamGroup] = {}
        n = 0
        for name in self.train:
            params = _model_params(model, name)
            g = ParamGroup(params, [tuple(p.shape) for p in params], n, sum(p.numel() for p in params), *_GROUPS[name])
            if name == "box" and g.shapes != list(ops.BOX_HEAD_SHAPES):
                raise NotImplementedError("HeadTrainer(train=('box', ..)): the box head is not the MLP 256 -> 256 -> 256 -> 4")
            if name == "tail" and (g.shapes != list(ops.tail_shapes(self.F)) or self.D != 256):
                raise NotImplementedError("HeadTrainer(train=('tail', ..)): the tail is not linear1 [F,256], linear2 [256,F], norm3 [256], decoder.norm [256]")
            if name == "cross" and (tuple(g.shapes) != ops.CROSS_SHAPES or self.D != 256):
                raise NotImplementedError("HeadTrainer(train=('cross', ..)): the block is not sampling_offsets [256,256], attention_weights [128,256], "
                                          "output_proj [256,256], norm1 [256]")
            if name == "self" and (tuple(g.shapes) != ops.SELF_SHAPES or self.D != 256):
                raise NotImplementedError("HeadTrainer(train=('self', ..)): the block is not in_proj [768,256], out_proj [256,256], norm2 [256]")
            if name == "value" and (g.shapes != [(256, 256), (256,)] or self.D != 256):
                raise NotImplementedError("HeadTrainer(train=('value', ..)): the block is not value_proj [256,256] with its bias [256]")
            self.groups[name] = g
            n += g.n
        self.n_class, self.n_box, self.n_tail, self.n_cross, self.n_self, self.n_value = (self.groups[k].n if k in self.groups else 0 for k in TRAINABLE_FULL)
        dev = head.weight.device
        self.param = torch.cat([p.detach().float().reshape(-1) for g in self.groups.values() for p in g.params]).to(dev).contiguous()
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.scale = torch.ones(2, dtype=torch.float32, device=dev)         # (clip coefficient, gradient norm) of the last step
        self.step_count = 0
        self.last_outputs: Optional[Dict[str, torch.Tensor]] = None         # pred_logits / pred_boxes of the last step (before its update)
        self.last_states: Optional[Dict] = None                             # hs_all, tgt_all, refs, stacked outputs, match_q of the last step

    # -- the masters: views of the flat buffer -------------------------------------------------------------------------------------
    def _views(self, name: str, untrained: str) -> List[torch.Tensor]:
        if name not in self.groups:
            raise RuntimeError(untrained)
        return self.groups[name].views(self.param)

    @property
    def weight(self) -> torch.Tensor:
        return self.groups["class"].views(self.param)[0] if self.n_class else self.model.class_embed[0].weight.detach()

    @property
    def bias(self) -> torch.Tensor:
        return self.groups["class"].views(self.param)[1] if self.n_class else self.model.class_embed[0].bias.detach()

    def box_head(self) -> List[torch.Tensor]:
        """the master box head as views of the flat buffer: [W0, b0, W1, b1, W2, b2] (train includes "box")"""
        return self._views("box", "HeadTrainer: the box head is not trained (train=('class',))")

    def tail(self) -> List[torch.Tensor]:
        """the master tail as views of the flat buffer: [W1, b1, W2, b2, norm3.w, norm3.b, dec_norm.w, dec_norm.b] (train includes "tail")"""
        return self._views("tail", "HeadTrainer: the decoder tail is not trained (train lacks 'tail')")

    def cross(self) -> List[torch.Tensor]:
        """the master cross-attention block as views of the flat buffer: [so.W, so.b, aw.W, aw.b, out.W, out.b, norm1.w, norm1.b] (train
        includes "cross")"""
        return self._views("cross", "HeadTrainer: the cross-attention block is not trained (train lacks 'cross')")

    def self_block(self) -> List[torch.Tensor]:
        """the master self-attention block as views of the flat buffer: [in_proj.W, in_proj.b, out_proj.W, out_proj.b, norm2.w, norm2.b]
        (train includes "self")"""
        return self._views("self", "HeadTrainer: the self-attention block is not trained (train lacks 'self')")

    def value_proj(self) -> List[torch.Tensor]:
        """the master value projection as views of the flat buffer: [value_proj.W, value_proj.b] (train includes "value")"""
        return self._views("value", "HeadTrainer: the value projection is not trained (train lacks 'value')")

    def _box_weights(self) -> List[torch.Tensor]:
        """the box MLP the forward runs: the master when it is trained, else the model's"""
        return self.box_head() if self.n_box else [p.detach().float() for p in _model_params(self.model, "box")]

    def _engine(self):
        eng = self.model.engine()
        for g in self.groups.values():
            g.attach(eng, g.views(self.param))
        return eng

    # -- steps -------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def cache(self, samples, per_line: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """(hs [B,nq,hidden] in the engine's dtype, pred_boxes [B,nq,4]) of a batch: the frozen trunk's part of a step.  With "tail"
        trained the trunk ends one block earlier: (tail_in [B,nq,hidden], the last decoder layer's FFN input, and ref_last [B,nq,4], that
        layer's reference points)."""
        self._no_cache("cache")
        self._engine()
        if self.n_tail:                                                     # (the last layer's FFN input, its reference points): tail_forward's arguments
            out = self.model(samples, per_line=per_line, return_hidden="tail")
            return out["tail_in"], out["refs"][len(out["hs_all"]) - 1]
        out = self.model(samples, per_line=per_line, return_hidden=True)
        return out["hs"], out["pred_boxes"]

    @torch.no_grad()
    def step(self, samples, target_labels: Sequence[Sequence[int]], per_line: bool = False, target_boxes=None) -> Dict[str, torch.Tensor]:
        """One training step through the full forward (engine.train_one_epoch_CTC's loop body, engine.py:190-216)."""
        self._engine()
        if self.every_output:
            out = self.model(samples, per_line=per_line, return_hidden="value" if self.n_value else "self" if self.n_self else "cross" if self.n_cross else "tail" if self.n_tail else "all")
        else:                                                               # the class head on the main output: the last state is all the step reads
            o = self.model(samples, per_line=per_line, return_hidden=True)
            out = self._main_output(o["hs"], o["pred_logits"], o["pred_boxes"])
        return self._update(out, target_labels, target_boxes)

    @torch.no_grad()
    def step_cached(self, hs: torch.Tensor, boxes: torch.Tensor, target_labels: Sequence[Sequence[int]], target_boxes=None) -> Dict[str, torch.Tensor]:
        """The same step on cached decoder states: only the class head runs forward -- with "tail" trained, on cache()'s (tail_in,
        ref_last): the last FFN, the norms and both heads run forward (DTLREngine.tail_forward), in the bits of the full step."""
        self._no_cache("step_cached")
        if self.n_tail:                                                     # hs, boxes: cache()'s (tail_in, ref_last)
            o = self._engine().tail_forward(hs, boxes)
            out = self._main_output(o["hs"], o["pred_logits"], o["pred_boxes"], ref=boxes, tail_in=hs)
        else:
            out = self._main_output(hs, self._engine()._class_head(hs), boxes)
        return self._update(out, target_labels, target_boxes)

    @staticmethod
    def _main_output(hs, logits, boxes, ref=None, **more):
        """what return_hidden="all" would hold of a decoder with the main output alone (L = 1); ref: that output's reference points,
        which only the box gradient reads"""
        return {"hs_all": [hs], "tgt_all": [None], "refs": [ref], "aux_outputs": [], "pred_logits": logits, "pred_boxes": boxes, **more}

    def _no_cache(self, what):
        if "value" in self.train:
            raise ValueError(f"HeadTrainer.{what}: the value projection reads the decoder's memory, which the cache does not hold -- use step()")
        if "self" in self.train:
            raise ValueError(f"HeadTrainer.{what}: the self-attention block reads the layer's input state and runs the whole last layer, which the "
                             "cache does not hold -- use step()")
        if "cross" in self.train:
            raise ValueError(f"HeadTrainer.{what}: the cross-attention block reads the batch's value map, which the cache does not hold -- use step()")
        if "box" in self.train:
            raise ValueError(f"HeadTrainer.{what}: the forward depends on the box head being trained -- use step()")
        if self.aux_loss:
            raise ValueError(f"HeadTrainer.{what}: aux_loss needs every decoder layer's states, the cache holds the last layer's -- use step()")

    def _set_targets(self, target_labels, target_boxes, device):
        if target_boxes is None:
            raise ValueError(f"HeadTrainer(loss={self.loss!r}): the step needs target_boxes")
        return ops.set_targets([{"labels": torch.as_tensor(l, dtype=torch.int64), "boxes": torch.as_tensor(b, dtype=torch.float32).reshape(-1, 4)}
                                for l, b in zip(target_labels, target_boxes)], device, self.C)

    def _update(self, out, target_labels, target_boxes):
        """THE step, over the L decoder outputs `out` holds (return_hidden="all" / "tail", or _main_output's L = 1): the losses, dW of
        the class head summed over the weighted outputs, the box head's gradient at its 2 L - 1 applications, the tail's chain, then one
        clip and one AdamW over the flat buffer.  With L = 1 and the class head alone this is the four-operator chain of the module
        docstring: nothing is stacked or concatenated, the set losses see one row of weights."""
        hs_all, tgt_all, refs = out["hs_all"], out["tgt_all"], out["refs"]
        L = len(hs_all)
        logits = _cat([a["pred_logits"][None] for a in out["aux_outputs"]] + [out["pred_logits"][None]])
        boxes = _cat([a["pred_boxes"][None] for a in out["aux_outputs"]] + [out["pred_boxes"][None]])
        B, nq = int(logits.shape[1]), int(logits.shape[2])
        self.last_outputs = {"pred_logits": out["pred_logits"], "pred_boxes": out["pred_boxes"]}
        used = [l for l in range(L) if self.aux_loss or l == L - 1]
        cls_on, box_on = bool(self.n_class or self.n_tail), bool(self.n_box or self.n_tail)      # the tail moves both outputs through the states
        self.last_states = {"hs_all": hs_all, "tgt_all": tgt_all, "refs": refs, "pred_logits": logits, "pred_boxes": boxes}
        if self.n_tail:
            self.last_states["tail_in"] = out["tail_in"]
        if self.n_cross:
            self.last_states["cross_in"] = out["cross_in"]
        if self.n_self:
            self.last_states["self_in"] = out["self_in"]
        if self.n_value:
            self.last_states["value_in"] = out["value_in"]
        match = r = None
        if self.loss == "ctc":                                                  # the CTC loss reaches the tail through dlogits alone
            result = {}
            result["loss_CTC"], dctc = E.loss_ctc_backward(self.last_outputs, target_labels)
            dlogits = {L - 1: dctc}
        else:
            tg = self._set_targets(target_labels, target_boxes, logits.device)
            match = self.matcher.match(logits, boxes, tg)
            self.last_states["match_q"] = match
            row = [self.cls_loss_coef if cls_on else 0.0, self.bbox_loss_coef if box_on else 0.0, self.giou_loss_coef if box_on else 0.0]
            r = ops.set_loss(logits, boxes, tg, match, max(float(sum(tg.sizes)), 1.0), [row if l in used else [0.0, 0.0, 0.0] for l in range(L)],
                             [cls_on and l in used for l in range(L)], self.matcher.focal_alpha)
            v = r["losses"]
            result = {"loss_ce": v[L - 1, 0], "loss_bbox": v[L - 1, 1], "loss_giou": v[L - 1, 2], "cardinality_error": v[L - 1, 5], "class_error": v[L - 1, 6]}
            for l in range(L - 1):
                result.update({f"loss_ce_{l}": v[l, 0], f"loss_bbox_{l}": v[l, 1], f"loss_giou_{l}": v[l, 2]})
            if self.loss == "ctc+set":
                if cls_on:
                    result["loss_CTC"], dctc = E.loss_ctc_backward(self.last_outputs, target_labels)
                    r["dlogits"][L - 1].add_(dctc, alpha=self.CTC_loss_coef)
                else:
                    result["loss_CTC"] = E.loss_ctc(self.last_outputs, target_labels)
            dlogits = {l: r["dlogits"][l] for l in used} if cls_on else {}
        G = _cat([dlogits[l].view(-1, self.C) for l in used]) if dlogits else None
        if self.n_class:
            ops.head_grad(G, _cat([hs_all[l].reshape(-1, self.D) for l in used]), out=self.groups["class"].of(self.grad))
        dz = None
        if box_on and r is not None:
            dz, du = ops.box_refine_grad(r["dboxes"], boxes, torch.stack(refs[:L]))
        if self.n_box:
            below = [l for l in used if l >= 1]                                  # look forward twice: output l's box also reads f(t_(l-1))
            xs = [hs_all[l].reshape(-1, self.D) for l in used] + [tgt_all[l - 1].reshape(-1, self.D) for l in below]
            dys = [dz[l] for l in used] + [du[l - 1] for l in below]
            rows = ops.match_rows(match, nq, B)[used + below]
            ops.box_mlp_grad(xs, dys, self.box_head(), rows=rows, out=self.groups["box"].of(self.grad))
        if self.n_tail:
            # the gradient at h_l of every weighted output: the class head's input gradient, plus the box MLP's on the matched rows;
            # the terms at t_(l-1) (look forward twice) land on frozen states and are dropped
            M = B * nq
            dh = ops.head_dx(G, self.weight) if G is not None else torch.zeros((len(used) * M, self.D), dtype=torch.float32, device=logits.device)
            if dz is not None:
                ops.box_mlp_dx([hs_all[l].reshape(-1, self.D) for l in used], [dz[l] for l in used], [dh[k * M:(k + 1) * M] for k in range(len(used))],
                               self._box_weights(), rows=ops.match_rows(match, nq, B)[used])
            t_below = [tgt_all[l] for l in used if l < L - 1]
            if self.n_cross:
                # the block below the tail: everything from the state after norm2 upward is recomputed in fp32 from the masters, the tail's
                # chain starts from that u and hands back the gradient at it
                ci = out["cross_in"]
                s, qpos, rec_s = ci["s"], ci["qpos"], None
                if self.n_self:
                    # one block deeper: the state after norm2 is recomputed in fp32 from the layer's input and the masters, and the cross
                    # block starts from that s (its query position embedding cast up: one dtype for both)
                    si = out["self_in"]
                    rec_s = ops.self_recompute(si["t"], si["qpos"], self.self_block())
                    s, qpos = rec_s["s"].view(B, nq, self.D), qpos.float()
                if self.n_value:
                    # the layer's value map in fp32 from the master, the rows under the padding mask zero as the forward fills them: the
                    # cross block samples THIS map, not the engine's slice
                    vi = out["value_in"]
                    Wv, bv = self.value_proj()
                    mem = vi["memory"].reshape(-1, self.D).float()
                    Vf = ops.head_dx(mem, Wv.t().contiguous()).add_(bv)
                    if vi["mask"] is not None:
                        Vf.masked_fill_(vi["mask"].reshape(-1, 1), 0.0)
                    ci = dict(ci, value=Vf.view(B, -1, 8, self.D // 8))
                rec = ops.cross_recompute(s, qpos, ci["ref_in"], ci["value"], ci["shapes"], ci["lsi"], self.cross())
                _, grad_u = ops.tail_grad(rec["u"], t_below, dh, self.tail(), out=self.groups["tail"].of(self.grad), return_du=True)
                if rec_s is None:
                    ops.cross_grad(ci, rec, grad_u, self.cross(), out=self.groups["cross"].of(self.grad))
                elif not self.n_value:
                    _, grad_s = ops.cross_grad(ci, rec, grad_u, self.cross(), out=self.groups["cross"].of(self.grad), return_ds=True)
                    ops.self_grad(si, rec_s, grad_s, self.self_block(), out=self.groups["self"].of(self.grad))
                else:
                    _, grad_s, grad_o = ops.cross_grad(ci, rec, grad_u, self.cross(), out=self.groups["cross"].of(self.grad), return_ds=True,
                                                       return_do=True)
                    ops.self_grad(si, rec_s, grad_s, self.self_block(), out=self.groups["self"].of(self.grad))
                    dV = ops.msda_value_grad(ci["shapes"], ci["lsi"], rec["loc"], rec["A"], grad_o.view(B, nq, self.D), int(Vf.shape[0]) // B)
                    dV = dV.view(-1, self.D)
                    if vi["mask"] is not None:
                        dV.masked_fill_(vi["mask"].reshape(-1, 1), 0.0)
                    ops.head_grad(dV, mem, out=self.groups["value"].of(self.grad))         # [dWv | dbv]: value_proj as a head of 256 "classes"
            else:
                ops.tail_grad(out["tail_in"], t_below, dh, self.tail(), out=self.groups["tail"].of(self.grad))
        clip = self.max_norm > 0
        if clip:
            ops.grad_norm_scale(self.grad, self.max_norm, out=self.scale)
        self.step_count += 1
        ops.adamw_step(self.param, self.exp_avg, self.exp_avg_sq, self.grad, self.step_count, self.lr, self.betas, self.eps,
                       self.weight_decay, grad_scale=self.scale if clip else None)
        return result

    # -- state -------------------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict:
        """"head" / "exp_avg" / "exp_avg_sq": the class head [W | b] and its moments, as before the box head could be trained (without
        "class" in train: the model's head and empty moments); "box_head" / "box_exp_avg" / "box_exp_avg_sq" and "tail" / "tail_exp_avg" /
        "tail_exp_avg_sq": the same of the box head [W0 | b0 | W1 | b1 | W2 | b2] and of the tail [W1 | b1 | W2 | b2 | norm3.w | norm3.b |
        dec_norm.w | dec_norm.b], present when they are trained; "cross" / "cross_exp_avg" / "cross_exp_avg_sq": likewise the cross-attention
        block [so.W | so.b | aw.W | aw.b | out.W | out.b | norm1.w | norm1.b]; "self" / "self_exp_avg" / "self_exp_avg_sq": the self-attention
        block [in_proj.W | in_proj.b | out_proj.W | out_proj.b | norm2.w | norm2.b]; "value" / "value_exp_avg" / "value_exp_avg_sq": the last
        decoder layer's value projection [value_proj.W | value_proj.b]."""
        t = {key: g.of(flat).detach().cpu().clone() for g in self.groups.values() for key, flat in zip(g.keys, (self.param, self.exp_avg, self.exp_avg_sq))}
        if not self.n_class:
            t.update(head=torch.cat([self.weight.reshape(-1), self.bias.reshape(-1)]).detach().float().cpu().clone(),
                     exp_avg=torch.zeros(0), exp_avg_sq=torch.zeros(0))
        sd = {key: t.pop(key) for key in _GROUPS["class"][0]}
        sd.update({"step": int(self.step_count), "num_classes": self.C, "hidden_dim": self.D})
        if t:
            sd.update({"train": list(self.train), **t})
        if self.n_tail:
            sd["dim_feedforward"] = self.F
        return sd

    def load_state_dict(self, sd: Dict) -> None:
        if int(sd["num_classes"]) != self.C or int(sd["hidden_dim"]) != self.D:
            raise ValueError(f"HeadTrainer.load_state_dict: the state is of a Linear({sd['hidden_dim']} -> {sd['num_classes']}), "
                             f"this trainer's head is Linear({self.D} -> {self.C})")
        for g in self.groups.values():
            key, m, v = g.keys
            if key not in sd:                                               # a state written before this group could be trained: it stays
                continue                                                    # the model's, its moments zero
            if sd[key].numel() != g.n:
                raise ValueError(f"HeadTrainer.load_state_dict: the state's {key} has {sd[key].numel()} elements, this trainer's {g.n}")
            g.of(self.param).copy_(sd[key])
            if sd[m].numel():                                               # empty: written by a trainer that did not train the class head
                g.of(self.exp_avg).copy_(sd[m])
                g.of(self.exp_avg_sq).copy_(sd[v])
        self.step_count = int(sd["step"])

    @torch.no_grad()
    def write_back(self):
        """Copy the master heads into model.class_embed (the shared Linear) and, when trained, model.bbox_embed (the shared MLP: every
        aliased state-dict key carries the new values): model.state_dict() then is the adapted checkpoint."""
        for g in self.groups.values():
            for p, v in zip(g.params, g.views(self.param)):
                p.copy_(v)
        self.model._engine = None                                           # the packed model is rebuilt from the new parameters
        return self.model


# ------------------------------------------------------------------------------------------------------------------------- CLI
def build_parser() -> argparse.ArgumentParser:
    from .transforms import EVAL_MAX_SIZE, EVAL_SIZE
    ap = argparse.ArgumentParser(prog="python -m dtlr_amd.adapt",
                                 description="train the class head of a pretrained DTLR checkpoint for a new charset (CTC loss, AdamW), on the GPU")
    ap.add_argument("--config", default="latin", help="a reference config file (config/*.py) or a preset: latin | chinese | tiny")
    ap.add_argument("--weights", required=True, help="the pretrained checkpoint.pth")
    ap.add_argument("--images", default=None, help="folder with the line images (<id>.jpg / .png); required unless the lines are synthetic")
    ap.add_argument("--labels", default=None, help="labels.pkl (reference layout), .json or .tsv; required unless the lines are synthetic")
    ap.add_argument("--mode", default="train", help="split of a labels.pkl")
    ap.add_argument("--charset", required=True, help="the NEW charset (.json list / .pkl list)")
    ap.add_argument("--old-charset", default=None, help="charset of the checkpoint (--smart-mapping; default: the package's default_charset.json)")
    ap.add_argument("--smart-mapping", action="store_true", help="initialise the new head from the old head's rows (finetuning.py --smart_mapping)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the head initialisation and of the batch order")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--epochs", type=int, default=None)
    g.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--batching", default="exact", choices=["exact", "padded", "ragged"])
    ap.add_argument("--cache-features", action="store_true", help="run the frozen trunk once per batch and train on the cached decoder states")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32s", "f32"])
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--weight-decay", type=float, default=1e-4)
    ap.add_argument("--clip-max-norm", type=float, default=0.01, help="<= 0: no clipping")
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--limit", type=int, default=0, help="train on the first N lines only")
    ap.add_argument("--size", type=int, default=EVAL_SIZE)
    ap.add_argument("--max_size", type=int, default=EVAL_MAX_SIZE)
    ap.add_argument("--loss", default="ctc", choices=["ctc", "set", "ctc+set"],
                    help="ctc: the CTC loss (default); set: Hungarian matching against character boxes + the focal loss; ctc+set: both")
    ap.add_argument("--boxes-from", default="labels", choices=["labels", "align"],
                    help="where the set loss's character boxes come from: labels = the --boxes file; align = the CTC forced alignment of "
                         "each transcript under the initial head (evaluation.align_ctc), lines without a feasible alignment are skipped")
    ap.add_argument("--boxes", default=None, help="JSON {image id: [[cx, cy, w, h], ...]}: one box a character, normalised to 0..1 (--boxes-from labels)")
    ap.add_argument("--train", default="class", help="the heads to train, comma-separated: class (default), box (the shared box head; needs "
                                                     "--loss set or ctc+set and the full forward every step), tail (the last decoder "
                                                     "layer's FFN and norm3 and decoder.norm; any loss), cross (that layer's cross-attention "
                                                     "and norm1; needs tail and the full forward every step), self (that layer's "
                                                     "self-attention and norm2; needs cross), value (that layer's cross_attn.value_proj; "
                                                     "needs self), e.g. class,box,tail,cross,self,value")
    ap.add_argument("--aux-loss", action="store_true", help="set losses on every decoder output, as the reference weighs them (default: the main output)")
    ap.add_argument("--augment", default="none", choices=["none", "default", "full"],
                    help="the reference's training erasing, on the device (DESIGN.md section 26): none (default: the evaluation transform); default: "
                         "4 x RandomErasing(p 0.5, scale 0.005-0.05, ratio 5-6); full: 5 full-height bars of 1-4 %% of the width in front of "
                         "those (the reference's --random_erasing)")
    ap.add_argument("--aug-scales", default=None, help="comma-separated short sides, one drawn per line and step (the reference's data_aug_scales); "
                                                       "default: no random resize; needs --batching padded or ragged")
    ap.add_argument("--aug-seed", type=int, default=None, help="seed of the augmentation draws (default: --seed); a line's draws depend on "
                                                               "(seed, epoch, line) alone")
    ap.add_argument("--resident", action="store_true", help="decode every line once into one device buffer and feed every step from it")
    ap.add_argument("--resident-max-gb", type=float, default=16.0, help="refuse --resident beyond this many GB of pixels")
    ap.add_argument("--val-labels", default=None, help="labels of held-out lines: val loss_CTC and val CER at the end of every epoch and of the run")
    ap.add_argument("--val-mode", default=None, help="split of the held-out lines in a labels.pkl (default val; with no --val-labels: a split of --labels)")
    ap.add_argument("--val-images", default=None, help="folder of the held-out lines' images (default: --images)")
    ap.add_argument("--synth-fonts", default=None, help="train on synthetic lines rendered on the device (DESIGN.md section 27): comma-separated "
                                                        ".ttf / .otf paths, or builtin (Pillow's default face); every character carries its box")
    ap.add_argument("--synth-atlas", default=None, help="the same from a glyph atlas written by synthlines.GlyphAtlas.save (no font needed)")
    ap.add_argument("--synth-text", default=None, help="a text file, one line a line (default: 1-5 random words over --charset)")
    ap.add_argument("--synth-lines", type=int, default=None, help="lines of the synthetic set; every epoch renders fresh ones")
    ap.add_argument("--synth-font-sizes", default=None, help="a size or a range of sizes (default 30-50, the reference's)")
    ap.add_argument("--synth-backgrounds", default=None, help="folder of background images kept on the device (default: procedural backgrounds)")
    ap.add_argument("--synth-seed", type=int, default=None, help="seed of the generator's draws (default: --seed); a line's draws depend on "
                                                                 "(seed, epoch, line) alone")
    ap.add_argument("--out", required=True, help="the adapted checkpoint ({'model': state_dict, 'charset', 'trainer'})")
    return ap


def check_synth_args(ap: argparse.ArgumentParser, args) -> Optional[List[int]]:
    """The --synth-* flags against each other and the rest: None without them (--images / --labels are then demanded), otherwise the
    font sizes.  Every refusal is the parser's error, before anything is loaded."""
    synth = args.synth_fonts is not None or args.synth_atlas is not None
    if not synth:
        for name in ("synth_text", "synth_lines", "synth_font_sizes", "synth_backgrounds", "synth_seed"):
            if getattr(args, name) is not None:
                ap.error(f"--{name.replace('_', '-')} needs --synth-fonts or --synth-atlas")
        if args.images is None or args.labels is None:
            ap.error("the following arguments are required: --images, --labels (or --synth-fonts / --synth-atlas for synthetic lines)")
        return None
    if args.synth_fonts is not None and args.synth_atlas is not None:
        ap.error("--synth-fonts and --synth-atlas exclude each other")
    if args.images is not None or args.labels is not None or args.limit:
        ap.error("synthetic lines have no files: not with --images, --labels or --limit (held-out real lines: --val-images, --val-labels)")
    if args.synth_lines is None or args.synth_lines <= 0:
        ap.error("--synth-lines must be given and positive")
    if args.cache_features:
        ap.error("--cache-features cannot train on synthetic lines: every epoch renders fresh ones")
    if args.boxes_from != "labels" or args.boxes is not None:
        ap.error("synthetic lines carry the generator's boxes: not with --boxes or --boxes-from align")
    if args.val_mode is not None and args.val_labels is None:
        ap.error("--val-mode needs --val-labels with synthetic lines: there is no --labels file to take a split of")
    if (args.val_labels is not None) and args.val_images is None:
        ap.error("--val-labels needs --val-images with synthetic lines: there is no --images folder")
    from .synthlines import parse_range
    try:
        return parse_range(args.synth_font_sizes or "30-50")
    except ValueError:
        ap.error(f"--synth-font-sizes {args.synth_font_sizes}: a size or a range such as 30-50")


def parse_scales(text: Optional[str]) -> Optional[List[int]]:
    """--aug-scales: "480,512" -> [480, 512]; None stays None; ValueError for anything but positive integers"""
    if text is None:
        return None
    scales = [int(t) for t in text.split(",") if t.strip()]
    if not scales or min(scales) <= 0:
        raise ValueError(text)
    return scales


def text_to_labels(text: str, charset: Sequence) -> List[int]:
    index = {ch: i for i, ch in reversed(list(enumerate(charset)))}
    try:
        return [index[ch] for ch in text]
    except KeyError as e:
        raise ValueError(f"character {e.args[0]!r} of a transcription is not in the charset") from None


def save_checkpoint(path: str, model, charset: Sequence, trainer: Optional[HeadTrainer] = None) -> None:
    ck = {"model": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "charset": list(charset)}
    if trainer is not None:
        ck["trainer"] = trainer.state_dict()
    torch.save(ck, path)


def load_char_boxes(args, trainer: HeadTrainer, rows, labels, batches, load_batch, per_line: bool):
    """The set loss's targets: line index -> [T,4] cxcywh boxes in 0..1, one a label, and the batches without the lines that have none.
    --boxes-from labels: the --boxes file.  --boxes-from align: the forced alignment of each transcript on the forward under the
    initial head (evaluation.align_ctc_records); a line whose transcript does not fit is skipped, the count goes to the log."""
    boxes: Dict[int, torch.Tensor] = {}
    if args.boxes_from == "labels":
        import json
        if not args.boxes:
            raise SystemExit("--loss set / ctc+set with --boxes-from labels needs --boxes")
        with open(args.boxes, encoding="utf-8") as f:
            table = json.load(f)
        for i, (name, _) in enumerate(rows):
            b = torch.as_tensor(table[name], dtype=torch.float32).reshape(-1, 4)
            if b.shape[0] != len(labels[i]):
                raise SystemExit(f"--boxes: {name} has {b.shape[0]} boxes for {len(labels[i])} characters")
            boxes[i] = b
        return boxes, batches
    skipped = 0
    trainer._engine()
    for idx in batches:
        with torch.no_grad():
            out = trainer.model(load_batch(idx), per_line=per_line)
        rec = E.align_ctc_records(out, [labels[i] for i in idx])
        lengths, xyxy = rec["lengths"].cpu().tolist(), rec["box"].cpu()
        for k, i in enumerate(idx):
            if lengths[k] < 0:
                skipped += 1
                continue
            b = xyxy[k, : lengths[k]]
            boxes[i] = torch.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], dim=1)
    print(f"--boxes-from align: {skipped} of {len(rows)} lines have no feasible alignment and are skipped", flush=True)
    kept = [[i for i in idx if i in boxes] for idx in batches]
    return boxes, [idx for idx in kept if idx]


def main(argv: Optional[Sequence[str]] = None) -> Dict:
    ap = build_parser()
    args = ap.parse_args(argv)
    train = tuple(k.strip() for k in args.train.split(",") if k.strip())
    if not train or set(train) - set(TRAINABLE_FULL):
        ap.error(f"--train {args.train}: a comma-separated subset of class, box, tail, cross, self, value")
    if "value" in train and "self" not in train:
        ap.error("--train value needs self: the gradient of the value projection passes through the cross-attention block either way")
    if "value" in train and args.cache_features:
        ap.error("--cache-features cannot train the value projection: it reads the decoder's memory")
    if "self" in train and "cross" not in train:
        ap.error("--train self needs cross: the gradient of the self-attention block passes through the cross-attention block either way")
    if "self" in train and args.cache_features:
        ap.error("--cache-features cannot train the self-attention block: it runs the whole last decoder layer")
    if "cross" in train and "tail" not in train:
        ap.error("--train cross needs tail: the gradient of the cross-attention block passes through the last FFN either way")
    if "cross" in train and args.cache_features:
        ap.error("--cache-features cannot train the cross-attention block: it reads the batch's value map")
    if "box" in train and args.cache_features:
        ap.error("--cache-features cannot train the box head: the forward depends on it")
    if ("box" in train or args.aux_loss) and args.loss == "ctc":
        ap.error("--train box / --aux-loss need --loss set or ctc+set")
    if args.aux_loss and args.cache_features:
        ap.error("--cache-features keeps the last decoder layer's states only: not with --aux-loss")
    try:
        scales = parse_scales(args.aug_scales)
    except ValueError:
        ap.error(f"--aug-scales {args.aug_scales}: a comma-separated list of positive integers")
    if scales is not None and args.batching == "exact":
        ap.error("--aug-scales needs --batching padded or ragged: the lines of a batch no longer share one size")
    if args.cache_features and (args.augment != "none" or scales is not None):
        ap.error("--cache-features cannot train on augmented lines: the cached states are those of one fixed image")
    if args.resident_max_gb <= 0:
        ap.error("--resident-max-gb must be positive")
    synth_sizes = check_synth_args(ap, args)
    from . import eval_harness as H
    from . import weights as W
    from .config import DTLRConfig
    from .dino import DINO
    from .transforms import ERASING_DEFAULT, ERASING_FULL, DeviceLineSet, EvalTransform, TrainTransform
    if not torch.cuda.is_available():
        raise SystemExit("dtlr_amd.adapt needs an MI355X (no CPU path)")
    dev = torch.device("cuda", torch.cuda.current_device())
    charset = H.load_charset(args.charset)
    sd = W.load_checkpoint_state_dict(args.weights)
    n_old = W.num_classes_of(sd)
    if args.config in ("latin", "chinese"):
        cfg = {"latin": DTLRConfig.latin, "chinese": DTLRConfig.chinese}[args.config]()
    elif args.config == "tiny":
        cfg = DTLRConfig.tiny(num_classes=n_old)
    else:
        cfg = DTLRConfig.from_reference_file(args.config)
    model = DINO(cfg, compute_dtype={"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f32s": "f32s"}[args.dtype])
    model = E.load_model(model, sd, device=dev, new_class_embedding=n_old != cfg.num_classes, charset_size=n_old, fix_enc_out_class=True)
    torch.manual_seed(args.seed)
    if args.smart_mapping:
        w0, b0 = smart_mapping_init(model.class_embed[0], H.load_charset(args.old_charset), charset, args.seed)
        new_class_head(model, len(charset), w0, b0)
    else:
        new_class_head(model, len(charset))
    trainer = HeadTrainer(model, lr=args.lr, weight_decay=args.weight_decay, max_norm=args.clip_max_norm, loss=args.loss,
                          train=train, aux_loss=args.aux_loss)

    synth = None
    if synth_sizes is not None:
        # synthetic lines: the set is rendered on the device, the labels and boxes come from its layout, and the
        # loop below renders fresh lines at the start of every epoch
        from . import synthlines as SL
        seed = args.seed if args.synth_seed is None else args.synth_seed
        synth = SL.SyntheticLineSet(SL.atlas_from_args(args.synth_fonts, args.synth_atlas, charset, synth_sizes, seed=seed),
                                    SL.SynthRecipe(font_size=(synth_sizes[0], synth_sizes[-1])), args.synth_lines, SL.read_text(args.synth_text),
                                    SL.load_backgrounds(args.synth_backgrounds), device=dev, max_bytes=int(args.resident_max_gb * 1e9), charset=charset,
                                    seed=seed, epoch=0)
        rows, paths = [(f"{i:06d}", None) for i in range(len(synth))], []
        labels, sizes = [synth.labels(i) for i in range(len(synth))], list(synth.hw)
    else:
        rows = H.load_labels(args.labels, args.mode)
        if args.limit:
            rows = rows[: args.limit]
        paths = [H.find_image(args.images, name) for name, _ in rows]
        labels = [text_to_labels(t, charset) for _, t in rows]
        sizes = [H.image_size(p) for p in paths]
    per_line = args.batching == "ragged"
    batches = H.plan_batches(sizes, args.batch, args.batching == "exact", args.size, args.max_size)
    tf = EvalTransform(args.size, args.max_size)
    # the training transform: None is the evaluation transform, the path before augmentation
    ttf = None
    if args.augment != "none" or scales is not None:
        ttf = TrainTransform(args.size, args.max_size, scales=scales, erasing={"none": (), "default": ERASING_DEFAULT, "full": ERASING_FULL}[args.augment],
                             seed=args.seed if args.aug_seed is None else args.aug_seed)
    val = None
    if args.val_labels is not None or args.val_mode is not None:
        vrows = H.load_labels(args.val_labels or args.labels, args.val_mode or "val")
        vpaths = [H.find_image(args.val_images or args.images, name) for name, _ in vrows]
        vsizes = [H.image_size(p) for p in vpaths]
        val = {"paths": vpaths, "labels": [text_to_labels(t, charset) for _, t in vrows], "set": None,
               "batches": H.plan_batches(vsizes, args.batch, args.batching == "exact", args.size, args.max_size)}
    lines = synth
    if synth is not None:
        if args.resident and val:
            val["set"] = DeviceLineSet([H.read_rgb(p) for p in val["paths"]], device=dev, max_bytes=int(args.resident_max_gb * 1e9))
    elif args.resident:
        cap = int(args.resident_max_gb * 1e9)
        need = sum(h * w * 3 for h, w in sizes + (vsizes if val else []))
        if need > cap:
            raise SystemExit(f"--resident: the lines hold {need / 1e9:.3f} GB of pixels, more than --resident-max-gb {args.resident_max_gb:g}")
        lines = DeviceLineSet([H.read_rgb(p) for p in paths], device=dev, max_bytes=cap)
        if val:
            val["set"] = DeviceLineSet([H.read_rgb(p) for p in val["paths"]], device=dev, max_bytes=cap - lines.nbytes)

    def eval_lines(idx):
        """the batch `idx` under the evaluation transform: from the resident set, or from the files"""
        return lines.eval_batch(idx, args.size, args.max_size) if lines is not None else tf([H.read_rgb(paths[i]) for i in idx], device=dev)

    def train_lines(idx, epoch):
        if ttf is None:
            return eval_lines(idx)
        return lines.train_batch(idx, ttf, epoch) if lines is not None else ttf([H.read_rgb(paths[i]) for i in idx], idx, epoch, device=dev)

    def validate():
        """the held-out lines, never augmented, through the forward with the parameters as they stand: (loss_CTC, CER) over the lines"""
        trainer._engine()
        loss = cer = n = 0.0
        for idx in val["batches"]:
            x = val["set"].eval_batch(idx, args.size, args.max_size) if val["set"] is not None else tf([H.read_rgb(val["paths"][i]) for i in idx], device=dev)
            with torch.no_grad():
                ev = E.evaluate_ctc_step(trainer.model(x, per_line=per_line), [val["labels"][i] for i in idx])
            loss, cer, n = loss + ev["loss_CTC"] * ev["n"], cer + ev["cer_sum"], n + ev["n"]
        return loss / max(n, 1), cer / max(n, 1)

    char_boxes: Dict[int, torch.Tensor] = {}
    if args.loss != "ctc" and synth is not None:
        char_boxes = {i: synth.boxes(i) for i in range(len(synth))}
    elif args.loss != "ctc":
        char_boxes, batches = load_char_boxes(args, trainer, rows, labels, batches, eval_lines, per_line)      # aligned on the un-augmented lines
    total = args.max_steps if args.max_steps is not None else (args.epochs if args.epochs is not None else 1) * len(batches)
    rng = np.random.Generator(np.random.PCG64(args.seed))
    cached: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}
    step, last, epoch = 0, {}, 0
    while step < total:
        if synth is not None and epoch > 0:                                   # fresh lines: sizes, labels and boxes follow the new layout
            synth.render(epoch)
            labels, sizes = [synth.labels(i) for i in range(len(synth))], list(synth.hw)
            batches = H.plan_batches(sizes, args.batch, args.batching == "exact", args.size, args.max_size)
            if args.loss != "ctc":
                char_boxes = {i: synth.boxes(i) for i in range(len(synth))}
        for bi in rng.permutation(len(batches)):
            if step >= total:
                break
            idx = batches[int(bi)]
            tl = [labels[i] for i in idx]
            tb = [char_boxes[i] for i in idx] if args.loss != "ctc" else None
            if args.cache_features:
                if int(bi) not in cached:
                    cached[int(bi)] = trainer.cache(eval_lines(idx), per_line=per_line)
                r = trainer.step_cached(*cached[int(bi)], tl, tb)
            else:
                r = trainer.step(train_lines(idx, epoch), tl, per_line=per_line, target_boxes=tb)
            step += 1
            if step % max(args.log_every, 1) == 0 or step == total:
                ev = E.evaluate_ctc_step(trainer.last_outputs, tl)            # the batch's loss and CER before this step's update
                last = {"step": step, **{k: float(v.item()) for k, v in r.items()}, "cer": ev["cer_sum"] / max(ev["n"], 1)}
                shown = "  ".join(f"{k} {last[k]:.6f}" for k in ("loss_CTC", "loss_ce", "loss_bbox", "loss_giou") if k in last)
                print(f"step {step}/{total}  {shown}  train CER {last['cer']:.4f}", flush=True)
        epoch += 1
        if val is not None:                                                   # the end of an epoch, or of the run inside one
            vloss, vcer = validate()
            last.update(val_loss_CTC=vloss, val_cer=vcer)
            print(f"epoch {epoch} (step {step}/{total})  val loss_CTC {vloss:.6f}  val CER {vcer:.4f}", flush=True)
    trainer.write_back()
    save_checkpoint(args.out, model, charset, trainer)
    print(f"wrote {args.out}", file=sys.stderr)
    return last


if __name__ == "__main__":
    main()

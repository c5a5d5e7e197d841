/* dtlr_setloss.h -- the set criterion of a DETR-style detector on the device, of libdtlr_hip.so (and libdtlr_hip_f16.so: the same code,
 * no 16-bit type is involved): the matching cost, the Hungarian assignment, and the focal / L1 / GIoU losses with their gradients.  A
 * seventh header beside dtlr_hip.h, under the same conventions: device pointers to contiguous buffers owned by the caller, work enqueued
 * on `stream` (a hipStream_t passed as void*; NULL = default stream) without synchronising, DTLR_OK (0) or a negative DTLR_E* code of
 * dtlr_hip.h returned, nothing thrown.
 *
 * The Python binding (dtlr_amd/_lib.py) reads this file with the reader it uses for dtlr_hip.h, so the file stays in the same small
 * dialect: plain C99; comments in the block form only; by-value parameters of type int, long, float or double, everything else a
 * pointer; returns int, long or const char *.
 */
#ifndef DTLR_SETLOSS_H
#define DTLR_SETLOSS_H

#include "dtlr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Shapes shared by the three entry points (csrc/set_loss.hip; semantics: DESIGN.md section 20).  L stacked outputs of B lines, problem
 * p = l * B + b, P = L * B <= 65535 (DTLR_ESHAPE otherwise).
 *   logits [L,B,nq,C] fp32 ; boxes [L,B,nq,4] fp32, (cx, cy, w, h).
 *   The targets of the B lines, shared by the L outputs: labels [n_targets] int32, offsets [B + 1] int32 (line b's targets are
 *   offsets[b] .. offsets[b + 1] - 1), tboxes [n_targets,4] fp32 (cx, cy, w, h).  Tmax >= 1: the largest target count, as the caller
 *   states it.  The kernels clamp every offset to [0, n_targets], every line to its first Tmax targets, every label to [0, C) and skip
 *   a match outside [0, nq): bad tables give wrong numbers, never a fault.
 *
 * dtlr_set_cost: cost [P,Tmax,nq] fp32, target-major: element (t, q) of problem p is the matching cost of query q against the line's
 *   target t,
 *     cost_bbox * sum_i |box_q[i] - tbox_t[i]|  +  cost_class * (alpha (1 - s)^2 (-log(s + 1e-8)) - (1 - alpha) s^2 (-log(1 - s + 1e-8)))
 *       -  cost_giou * GIoU(xyxy(box_q), xyxy(tbox_t)),        s = sigmoid(logits[q, label_t]),
 *     GIoU = I / (U + 1e-6) - (Ac - U) / (Ac + 1e-6) (intersection, union, the enclosing box's area: the reference's own form),
 *   evaluated in fp64 from the fp32 inputs and rounded once.  Only a line's own block is formed; logits[q, label] is read once per
 *   (problem, query, DISTINCT label of the line).  Rows t >= T of a problem are written as zeros: every element is written on every call.
 *   Tmax <= 2048 (24 bytes of LDS a target), else DTLR_ESHAPE.
 *
 * dtlr_hungarian: the minimum-cost assignment of each of P rectangular blocks, by shortest augmenting paths with duals (the algorithm of
 *   scipy.optimize.linear_sum_assignment), duals, path costs and sums in fp64 over the fp32 costs.  One workgroup a problem.
 *   cost [P,Rmax,ncols] fp32 ; sizes [P] int32: problem p uses rows 0 .. sizes[p] - 1 (clamped to [0, Rmax]) and all ncols columns.
 *   When sizes[p] > ncols the columns are assigned instead and min(sizes[p], ncols) rows are matched.
 *   match [P,Rmax] int32: the column assigned to row r, -1 for rows >= sizes[p] and for rows left out ; status [P] int32: 0 solved ;
 *   -1 the used part of the block holds a NaN or an infinity (the solver is not entered, the match row is all -1) ; -2 a loop bound was
 *   exhausted (cannot happen on finite costs; the match row is all -1).  Every loop of the solver runs a trip count that is uniform
 *   over the workgroup and bounded: min(rows, ncols) augmentations of at most min(rows, ncols) + 1 scan steps each.
 *   Among columns of equal path cost an unassigned one is taken first, then the lowest index.
 *   threads: the workgroup size, 256 or 1024 ; 0 = the default (1024: the faster of the two where measured).  LDS a problem: 13 min(Rmax, ncols) + 25 max(Rmax, ncols) bytes,
 *   at most 150 KB, else DTLR_ESHAPE.
 *
 * dtlr_set_loss: given match_q [P,Tmax] int32 (dtlr_hungarian's match over dtlr_set_cost's block: the query of target t, or -1),
 *   losses [L,8] fp32, per output l:  0 loss_ce = sum over (b, q, c) of the sigmoid focal loss (gamma 2, alpha; the matched query's
 *     one-hot class is its target's label, every other query is all background) / num_boxes ; 1 loss_bbox = sum over matched pairs of
 *     the L1 distance / num_boxes ; 2 loss_giou = sum of (1 - GIoU) / num_boxes ; 3 loss_xy, 4 loss_hw: the two halves of loss_bbox ;
 *     5 cardinality_error = mean over the lines of |#{q: argmax_c logits != C - 1} - T| ; 6 class_error = 100 - 100 * (matched queries
 *     whose argmax is their label) / (matched queries), 100 without a matched query ; 7 the number of matched pairs.
 *   weights [L,3] fp32 on the DEVICE: (w_ce, w_bbox, w_giou) of output l.  The gradients are those of
 *     sum_l (w_ce[l] loss_ce[l] + w_bbox[l] loss_bbox[l] + w_giou[l] loss_giou[l]):
 *   dboxes [L,B,nq,4] fp32: every element written, exact zeros in the rows of unmatched queries ; sign(0) = 0 in the L1 term, and a
 *     clamp at 0 passes the gradient where its argument is >= 0, as torch does ; ties inside GIoU's min / max are not specified.
 *   dl_slot [L] int32 on the DEVICE: the slice of dlogits that output l's gradient goes to, or -1 for an output that gets none ;
 *   dlogits [n_slots,B,nq,C] fp32 (NULL when every slot is -1): every element of a named slice is written.
 *   alpha < 0: no class balancing (both weights 1).  num_boxes > 0.
 *   The focal loss and its gradient are evaluated in fp32 an element, summed in fp64 ; the pair terms in fp64.  No float atomics: the
 *   workgroups leave partial sums in the workspace and one finishing workgroup an output adds them in a fixed order, so two calls on
 *   the same inputs give the same bits.  workspace: dtlr_set_loss_workspace_bytes(L, B, nq) bytes, 8-byte aligned. */
int dtlr_set_cost(const float *logits, const float *boxes, const int *labels, const int *offsets, const float *tboxes, int n_targets,
                  int L, int B, int nq, int C, int Tmax, float cost_class, float cost_bbox, float cost_giou, float alpha,
                  float *cost, void *stream);
int dtlr_hungarian(const float *cost, const int *sizes, int P, int Rmax, int ncols, int threads, int *match, int *status, void *stream);
long dtlr_set_loss_workspace_bytes(int L, int B, int nq);
int dtlr_set_loss(const float *logits, const float *boxes, const int *labels, const int *offsets, const float *tboxes, int n_targets,
                  const int *match_q, int L, int B, int nq, int C, int Tmax, float alpha, float num_boxes, const float *weights,
                  const int *dl_slot, float *dlogits, float *dboxes, float *losses, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DTLR_SETLOSS_H */

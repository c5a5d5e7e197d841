/* dtlr_metrics.h -- the edit-distance metrics of libdtlr_hip.so (and libdtlr_hip_f16.so: the same code, no 16-bit type is involved).  A
 * third header beside dtlr_hip.h and dtlr_lexicon.h, under the same conventions: device pointers to contiguous buffers owned by the
 * caller, work enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream) without synchronising, DTLR_OK (0) or a
 * negative DTLR_E* code of dtlr_hip.h returned, nothing thrown.
 *
 * The Python binding (dtlr_amd/_lib.py) reads this file with the reader it uses for dtlr_hip.h, into a table of its own, so the file
 * stays in the same small dialect: plain C99; comments in the block form only; by-value parameters of type int, long, float or double,
 * everything else a pointer; returns int, long or const char *.
 */
#ifndef DTLR_METRICS_H
#define DTLR_METRICS_H

#include "dtlr_hip.h"

#define DTLR_EDIT_MAX_LEN 4096

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Edit distance and alignment (csrc/edit_align.hip; semantics: DESIGN.md section 16): n pairs of int32 sequences (a_p, b_p) scored in
 * one launch, one wavefront per pair on a fixed grid (workgroup g takes pairs g, g + G, ...).
 *   a, b: the sequences of all pairs, flat, int32 (any value: labels, code points, word ids) ; a_off, b_off [n + 1] long on the DEVICE,
 *     non-decreasing: pair p is a[a_off[p] .. a_off[p + 1]) against b[b_off[p] .. b_off[p + 1]).  The offsets are the caller's: they
 *     must lie inside the buffers (dtlr_amd/metrics.py builds them) ;
 *   max_a, max_b: the longest a_p and the longest b_p, as the caller states them, 0..DTLR_EDIT_MAX_LEN, else DTLR_ESHAPE ; a longer
 *     sequence is cut to its first max_a (max_b) elements.
 * With D[i][0] = i, D[0][j] = j and D[i][j] = D[i-1][j-1] if a[i-1] == b[j-1], else 1 + min(D[i-1][j-1], D[i-1][j], D[i][j-1]):
 *   dist [n] int32: D[la][lb], the Levenshtein distance ;
 *   counts [n,3] int32: (insertions, deletions, substitutions) of the alignment that the walk back from (la, lb) takes: at (i, j), both
 *     positive, equal elements step to (i-1, j-1) ; otherwise a substitution to (i-1, j-1) if D[i-1][j-1] is the least of the three, else
 *     a deletion to (i-1, j) if D[i-1][j] <= D[i][j-1], else an insertion to (i, j-1) ; at i == 0 the j elements left of b are
 *     insertions, at j == 0 the i elements left of a are deletions.  ins + del + sub == dist ;
 *   want_ops != 0: the alignment itself.  n_ops [n] int32: its steps, lb + deletions <= la + lb ; ops: int32 pairs (i, j), pair p's
 *     steps in FORWARD order at ops[2 (a_off[p] + b_off[p] + k)], k < n_ops[p]: (i, j) = a[i] stands against b[j] (a match when they
 *     are equal, a substitution otherwise), (i, -1) = a[i] is deleted, (-1, j) = b[j] is inserted ; i and j count inside the pair.
 *     Entries beyond n_ops[p] are not written.  ops holds 2 (a_off[n] + b_off[n]) int32 ;
 *   want_ops == 0: n_ops, ops and workspace are not touched and may be NULL.
 * workspace (want_ops != 0): workspace_bytes >= dtlr_edit_align_workspace_bytes(n, max_a, max_b) = n slots of
 *   max_a * ceil(max_b / 16) * 4 bytes rounded up to 128 (a 2-bit move per cell, a row of b in 32-bit words), 128-byte aligned ; a
 *   smaller workspace_bytes is DTLR_ESHAPE.  0 bytes and NULL are accepted when max_a == 0 or max_b == 0.
 * n == 0: nothing is done.  A refusal enqueues nothing.  Asynchronous on `stream`; never synchronises. */
int dtlr_edit_align(const int *a, const long *a_off, const int *b, const long *b_off, int n, int max_a, int max_b, int want_ops,
                    int *dist, int *counts, int *n_ops, int *ops, void *workspace, long workspace_bytes, void *stream);
long dtlr_edit_align_workspace_bytes(int n, int max_a, int max_b);

#ifdef __cplusplus
}
#endif

#endif /* DTLR_METRICS_H */

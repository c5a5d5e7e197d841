/* dtlr_lexicon.h -- the lexicon decoder of libdtlr_hip.so (and libdtlr_hip_f16.so: the same code, no 16-bit type is involved).  A
 * second header beside dtlr_hip.h, under the same conventions: device pointers to contiguous buffers owned by the caller, work
 * enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream) without synchronising, DTLR_OK (0) or a negative DTLR_E*
 * code of dtlr_hip.h returned, nothing thrown.
 *
 * The Python binding (dtlr_amd/_lib.py) reads this file with the reader it uses for dtlr_hip.h, into a table of its own, so the file
 * stays in the same small dialect: plain C99; comments in the block form only; by-value parameters of type int, long, float or double,
 * everything else a pointer; returns int, long or const char *.
 */
#ifndef DTLR_LEXICON_H
#define DTLR_LEXICON_H

#include "dtlr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Lexicon decoding (csrc/lexicon.hip; semantics: DESIGN.md section 15): for every span of a batch, the H best words of a lexicon of W
 * words by their best CTC path over the span's frames.  The lexicon is a trie; one max-product pass over it scores all its words at
 * once, exactly (nothing is pruned).  One workgroup per span on a fixed grid of at most 2048 workgroups (workgroup g takes spans g,
 * g + G, ...), all spans in one launch.
 *   emissions [B,T,V] fp32 probabilities, channel 0 = the CTC blank, rows in reading order (what dtlr_blank_emissions writes) ;
 *     V <= 15360 (a frame's fp64 logs are held in LDS), else DTLR_ESHAPE ;
 *   spans [n,3] int32 on the DEVICE: (line, first frame, one past the last frame), clamped as dtlr_ctc_align clamps them: every line
 *     to [0, B), every frame to [0, T], every span to its first Tmax frames ; Tmax >= 0: the longest span, as the caller states it ;
 *   the trie, int32 on the DEVICE, n_nodes >= 1 nodes in breadth-first order, node 0 = the root (the empty string):
 *     parent [n_nodes]: parent[i] < i (clamped to [0, i)) ; chan [n_nodes]: the emission channel of the node's character, 1..V-1
 *     (clamped to [0, V)) ; node_word [n_nodes]: the word that ends at the node, 0..W-1, each word at one node, or -1 (clamped to
 *     [-1, W)) ; depth_start [max_depth + 2]: depth_start[d] = the first node of depth d, depth_start[max_depth + 1] = n_nodes
 *     (clamped to [1, n_nodes] and made non-decreasing) ; max_depth: the longest word, 0..64, else DTLR_ESHAPE.  A bad table gives a
 *     wrong record, never a fault ;
 *   prior [W] fp64 on the DEVICE or NULL (= zeros): natural-log priors, already weighted ;
 *   1 <= H <= 8, else DTLR_ESHAPE ;
 *   lp[t,c] = ln(max((double) E[t,c], 1e-30)), all scores fp64.  Every node carries nb (the path ends on the node's character) and b (on
 *     a blank after it); before frame 0 all are -inf except b(root) = 0.  Frame t, from the values of frame t - 1, p = parent[i]:
 *     nb'(i) = max(nb(i), b(p), nb(p) if chan[p] != chan[i]) + lp[t, chan[i]] ; b'(i) = max(b(i), nb(i)) + lp[t, 0] ; nb'(root) = -inf.
 *     The score of the word that ends at node i is max(nb(i), b(i)) after the span's last frame: dtlr_ctc_align's score of that word
 *     on the same span with interleaved = 0.  A word longer than its span, or one whose repeated characters leave no room for the
 *     blanks between them, has no path and is never returned ;
 *   order: descending key = score + prior[w], equal keys: the lower word id first.
 * Outputs, every element written on every call:
 *   count [n] int32: the number of words returned, 0..H ; word [n,H] int32: their ids in that order, padded with -1 ;
 *   score [n,H] fp64: their scores WITHOUT the prior, padded with 0 ;
 *   base [n] fp64: the sum over the span's frames, in frame order, of ln(max((double) max_c E[t,c], 1e-30)): score - base <= 0 is
 *     the log-likelihood ratio against the frame-wise argmax path, exactly 0 when the word is the span's collapsed argmax.  A span
 *     without frames: count 0, base 0.
 * workspace: dtlr_lexicon_decode_workspace_bytes(n, n_nodes, Tmax) bytes, 16-byte aligned: per workgroup two arrays of (nb, b), 32
 *   bytes a node (0 and NULL accepted when Tmax == 0).  n == 0: nothing is done.  Asynchronous on `stream`; never synchronises. */
int dtlr_lexicon_decode(const float *emissions, int B, int T, int V, const int *spans, int n, int Tmax,
                        const int *parent, const int *chan, const int *node_word, const int *depth_start, int n_nodes, int max_depth,
                        int W, const double *prior, int H, int *count, int *word, double *score, double *base,
                        void *workspace, void *stream);
long dtlr_lexicon_decode_workspace_bytes(int n, int n_nodes, int Tmax);

#ifdef __cplusplus
}
#endif

#endif /* DTLR_LEXICON_H */

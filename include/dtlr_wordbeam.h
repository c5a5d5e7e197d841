/* dtlr_wordbeam.h -- the word beam search of libdtlr_hip.so (and libdtlr_hip_f16.so: the same code, no 16-bit type is involved).  A
 * fourth header beside dtlr_hip.h, dtlr_lexicon.h and dtlr_metrics.h, under the same conventions: device pointers to contiguous buffers
 * owned by the caller, work enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream) without synchronising, DTLR_OK
 * (0) or a negative DTLR_E* code of dtlr_hip.h returned, nothing thrown.
 *
 * The Python binding (dtlr_amd/_lib.py) reads this file with the reader it uses for dtlr_hip.h, into a table of its own, so the file
 * stays in the same small dialect: plain C99; comments in the block form only; by-value parameters of type int, long, float or double,
 * everything else a pointer; returns int, long or const char *.
 */
#ifndef DTLR_WORDBEAM_H
#define DTLR_WORDBEAM_H

#include "dtlr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Word beam search (csrc/word_beam.hip; semantics: DESIGN.md section 17): CTC prefix beam search over whole lines, restricted to the
 * words of a dictionary with separators between them, scored by an optional WORD-level back-off n-gram.  It is dtlr_ngram_beam's
 * search (lp = ln(max((double) E, 1e-30)), the N best non-blank channels of a frame, the stay rules, merging of
 * the contributions to one label sequence, fp64 scores, the tie order of the cut) with a restricted set of extensions and a language
 * model term per completed word instead of per character.  One workgroup per span, all spans in one launch.
 *   emissions [B,T,V] fp32 probabilities, channel 0 = the CTC blank (what dtlr_blank_emissions writes) ;
 *   spans [n,3] int32 on the DEVICE: (line, first frame, one past the last frame), normally a whole line.  The kernel clamps every line
 *     to [0, B), every frame to [0, T] and every span to its first Tmax frames ; Tmax >= 0: the longest span, as the caller states it ;
 *     Lmax >= max(Tmax, 1) (DTLR_ESHAPE / DTLR_EINVAL otherwise) ;
 *   the dictionary of W >= 0 distinct words, each 1..64 channels in 1..V-1, as a trie on the DEVICE, n_nodes >= 1 nodes, node 0 = the root:
 *     the children of node i are nodes child_lo[i] .. child_hi[i] - 1 (clamped to [0, n_nodes]), sorted by chan (the emission channel
 *     of the child's character) ; node_word [n_nodes]: the word that ends at the node, 0..W-1, or -1 (clamped to [-1, W)) ;
 *     ahead [n_nodes] fp64: the largest unigram log10 P of any word at or below the node, 0 at the root ; max_depth: the longest word,
 *     0..64, else DTLR_ESHAPE ;
 *   cls [V] int32 on the DEVICE: 0 the blank, 1 a word character, 2 a separator ; a channel of any other class is never extended ;
 *   lm: NULL, or a HOST struct of DEVICE pointers to a packed back-off trie of order <= 6 (dtlr_hip.h, dtlr_ngram_lm) over WORDS: its
 *     "channel" of word id k is k + 1, <s> is W + 1, </s> is W + 2 (eos_tok = W + 2 or -1) ; a word the model does not know scores the
 *     <unk> unigram behind its context's back-offs ;
 *   a hypothesis is a label sequence p with (pb, pnb, lm), its trie node (the node of p's trailing run of word characters; the root when
 *     p is empty or ends in a separator) and its LM state (after p's completed words; bos_state when bos is set, else 0).  Extension by
 *     c, base as in dtlr_ngram_beam: cls[c] == 1: allowed iff the node has a child with channel c, which is the new node ; cls[c] == 2:
 *     allowed iff the node is the root or a word ends there; a word that ends completes: lm += w ln(10) log10 P(word | state), the
 *     state moves past the word, the new node is the root ;
 *   ranking: the K largest (pb' (+) pnb') + lm + w ln(10) ahead[node] are kept ; ahead counts as 0 without lm or with lookahead == 0,
 *     and is never part of a returned score ;
 *   the end of a span: a hypothesis is complete iff its node is the root or a word ends there; a pending word adds its LM term, then,
 *     with eos and lm, w ln(10) log10 P(</s> | state) ; the complete hypothesis with the largest (pb (+) pnb) + lm is returned ;
 *   K: beam, 1..64 (DTLR_ESHAPE otherwise) ; N: tokens extended per frame; N <= 0 or N >= V - 1: all of them.  N <= 1024 and the LDS
 *     image ~ 8 (K N + N + 64) + 12 KB <= 150 KB, V <= 65536 (DTLR_ESHAPE) ;
 *   labels_out [n,Lmax] int32 (channels, -1 padded), len_out [n] int32, score_out [n] fp64, every element written: a span whose final
 *     beam holds no complete hypothesis gets length -1, score -inf and labels all -1 ; a span without frames gets length 0 and the end
 *     terms alone ; n = 0 is a no-op ;
 *   workspace: the back-pointer arena, dtlr_word_beam_workspace_bytes(n, Tmax, K) bytes.
 * A bad table gives a wrong string, never a fault.  Asynchronous on `stream`; never synchronises. */
int dtlr_word_beam(const float *emissions, int B, int T, int V, const int *spans, int n, int Tmax,
                   const int *child_lo, const int *child_hi, const int *chan, const int *node_word, const double *ahead,
                   int n_nodes, int max_depth, int W, const int *cls,
                   const dtlr_ngram_lm *lm, double lm_weight, int K, int N, int bos, int eos, int lookahead,
                   int *labels_out, int Lmax, int *len_out, double *score_out, void *workspace, void *stream);
long dtlr_word_beam_workspace_bytes(int n, int Tmax, int K);

#ifdef __cplusplus
}
#endif

#endif /* DTLR_WORDBEAM_H */

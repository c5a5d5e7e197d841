/* dtlr_lm.h -- n-gram language model training of libdtlr_hip.so (and libdtlr_hip_f16.so: the same code, no 16-bit type is involved):
 * a device-wide radix sort of 64-bit keys, and the interpolated modified Kneser-Ney estimator built on it (semantics: DESIGN.md
 * section 18).  A fifth header beside dtlr_hip.h, dtlr_lexicon.h, dtlr_metrics.h and dtlr_wordbeam.h, under the same conventions:
 * device pointers to contiguous buffers owned by the caller, work enqueued on `stream` (a hipStream_t passed as void*; NULL = default
 * stream) without synchronising, DTLR_OK (0) or a negative DTLR_E* code of dtlr_hip.h returned, nothing thrown.  A refusal enqueues
 * nothing.  Row counts are long.
 *
 * The Python binding (dtlr_amd/_lib.py) reads this file with the reader it uses for dtlr_hip.h, into a table of its own, so the file
 * stays in the same small dialect: plain C99; comments in the block form only; by-value parameters of type int, long, float or double,
 * everything else a pointer; returns int, long or const char *.
 */
#ifndef DTLR_LM_H
#define DTLR_LM_H

#include "dtlr_hip.h"

#define DTLR_SORT_TILE 4096
#define DTLR_LM_MAX_ORDER 8
#define DTLR_LM_BOS 1
#define DTLR_LM_EOS 2
#define DTLR_LM_UNK 3

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * dtlr_sort_u64 (csrc/lm_sort.h): keys_out [n] = keys_in [n] (unsigned 64-bit) in ascending order of their low key_bits bits, stable;
 * the bits above key_bits must be 0 for the result to be the sorted keys.  A least-significant-digit radix sort, 8 bits a pass, over the
 * ceil(key_bits / 8) digits in use; a pass is a digit histogram per tile of DTLR_SORT_TILE keys, a scan of the [digit][tile] table
 * and a stable scatter.  keys_in is not written; keys_out must not overlap it.
 *   key_bits 1..64, 0 <= n < 2^31, else DTLR_ESHAPE ; n == 0: nothing is done.
 * workspace: workspace_bytes >= dtlr_sort_u64_workspace_bytes(n) = with T = ceil(n / DTLR_SORT_TILE) tiles:
 *   8 n rounded up to 256 (the second key buffer) + 1024 T (the table, 256 counters of 32 bits a tile) + 4 ceil(256 T / 4096) rounded
 *   up to 256 (the sums of the table's chunks); 0 for n == 0 ; 256-byte aligned ; a smaller workspace_bytes is DTLR_ESHAPE. */
int dtlr_sort_u64(const void *keys_in, void *keys_out, long n, int key_bits, void *workspace, long workspace_bytes, void *stream);
long dtlr_sort_u64_workspace_bytes(long n);

/* ---------------------------------------------------------------------------------------------
 * The estimator (csrc/lm_train.hip).  Token ids: 0 = pad, DTLR_LM_BOS = <s>, DTLR_LM_EOS = </s>, DTLR_LM_UNK = <unk>, then the words;
 * `bits` is the bit length of the largest id, 2..32 ; order 1..DTLR_LM_MAX_ORDER and order * bits <= 64, else DTLR_ESHAPE.
 *
 * dtlr_lm_keys: tokens [n] int32, the lines one after another, each as <s> w .. </s> -> keys [n] unsigned 64-bit: key i holds the
 * `order` tokens from position i on, the first in the most significant of the order * bits bits in use, pad from the first position
 * behind the line's </s> (or behind the stream) on: no window crosses a line.  A token is read in its low `bits` bits. */
int dtlr_lm_keys(const int *tokens, long n, int order, int bits, void *keys, void *stream);

/* dtlr_lm_count: keys [n] SORTED -> counts [order] long: counts[k - 1] = the distinct k-grams, a k-gram being the first k tokens of
 * a key whose k-th token is not pad.  0 <= n < 2^31. */
int dtlr_lm_count(const void *keys, long n, int order, int bits, long *counts, void *stream);

/* dtlr_lm_compact: keys [n] SORTED -> the tables of all orders, one after another, order 1 first: rows [total].
 *   grams [total] unsigned 64-bit: the k tokens of the row's k-gram, the first in the most significant of its k * bits bits, ascending
 *     within an order ; cnt [total] long: how often it occurs (c_k).
 *   Order 1 holds one row more than dtlr_lm_count counted: <unk>, count 0, at its sorted place (row 2, behind <s> and </s>, which every
 *   corpus of at least one line holds).  So total = 1 + the sum of counts, which the caller states, below 2^31 (else DTLR_ESHAPE) ; a
 *   row that would fall outside [0, total) is not written.
 * workspace: workspace_bytes >= dtlr_lm_compact_workspace_bytes(n, order) = with T = ceil((n + 1) / DTLR_SORT_TILE):
 *   4 order T rounded up to 256 (heads per order and tile) + 4 ceil(order T / 4096) rounded up to 256 ; 256-byte aligned ; a smaller
 *   workspace_bytes is DTLR_ESHAPE. */
int dtlr_lm_compact(const void *keys, long n, int order, int bits, long total, void *grams, long *cnt, void *workspace,
                    long workspace_bytes, void *stream);
long dtlr_lm_compact_workspace_bytes(long n, int order);

/* dtlr_lm_estimate: the tables of dtlr_lm_compact -> the model.  offs [order + 1] long on the DEVICE: order k is rows offs[k - 1] ..
 * offs[k], offs[0] = 0, offs[order] = total, non-decreasing (the caller's: counts, plus the <unk> row).
 *   adj [total] long: the adjusted counts a_k ; ids: order k's rows as [rows, k] int32, order after order (sum of rows * k values) ;
 *   logp, bo [total] double: log10 p and log10 back-off (0 for order `order` and for a row that is the context of nothing ; -99 for the
 *   unigram <s>) ;
 *   flags [2] int: flags[0] bit k - 1 set = order k took the fallback discounts (0.5, 1, 1.5) ; flags[1] != 0 = a shorter n-gram that
 *   must exist was not found (the tables are not those of a corpus): the results are then not a model.
 * workspace: workspace_bytes >= dtlr_lm_estimate_workspace_bytes(order) = 64 (order + 1) bytes: per order t_1..t_4 (long) and
 *   D(1)..D(3) (double), then the unigram denominator and back-off mass ; 64-byte aligned ; a smaller workspace_bytes is DTLR_ESHAPE.
 *   The caller may read t and D there after the call. */
int dtlr_lm_estimate(const void *grams, const long *cnt, const long *offs, int order, int bits, long total, long *adj, int *ids,
                     double *logp, double *bo, int *flags, void *workspace, long workspace_bytes, void *stream);
long dtlr_lm_estimate_workspace_bytes(int order);

#ifdef __cplusplus
}
#endif

#endif /* DTLR_LM_H */

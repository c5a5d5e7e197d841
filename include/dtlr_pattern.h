/* dtlr_pattern.h -- regular-expression decoding and spotting over the CTC lattice, of libdtlr_hip.so (and libdtlr_hip_f16.so: the same
 * code, no 16-bit type is involved).  A sixth header beside dtlr_hip.h, under the same conventions: device pointers to contiguous
 * buffers owned by the caller, work enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream) without synchronising,
 * DTLR_OK (0) or a negative DTLR_E* code of dtlr_hip.h returned, nothing thrown.
 *
 * The Python binding (dtlr_amd/_lib.py) reads this file with the reader it uses for dtlr_hip.h, into a table of its own, so the file
 * stays in the same small dialect: plain C99; comments in the block form only; by-value parameters of type int, long, float or double,
 * everything else a pointer; returns int, long or const char *.
 */
#ifndef DTLR_PATTERN_H
#define DTLR_PATTERN_H

#include "dtlr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * The automaton (csrc/pattern.hip; semantics: DESIGN.md section 19; host compiler and check: dtlr_amd/pattern.py).  A deterministic
 * automaton of n_states states, state 0 the start, and n_arcs arcs (src, chan, dst), int32 tables on the DEVICE:
 *   arc_src [n_arcs], arc_chan [n_arcs]: the arc's source state and emission channel 1..V-1 ; the arcs are sorted by (dst, src,
 *     chan) and that order is the arc id ; dst_start [n_states + 1]: the arcs into state q are dst_start[q] .. dst_start[q + 1] - 1,
 *     dst_start[n_states] = n_arcs ; accept [n_states]: non-zero for an accepting state.
 *   n_states 1..4096 and n_arcs <= 1 << 20, else DTLR_ESHAPE.  The kernels clamp arc_src to [0, n_states), arc_chan to [0, V),
 *   dst_start to [0, n_arcs] and keep every state's range non-decreasing, and clamp every back-pointer they follow: a bad table gives a
 *   wrong record, never a fault and never an unbounded loop.
 * emissions [B,T,V] fp32 probabilities, channel 0 = the CTC blank, rows in reading order (what dtlr_blank_emissions writes) ;
 *   V <= 15360 (a frame's fp64 logs are held in LDS), else DTLR_ESHAPE.
 * Every arc a carries nb(a) (the path's last frame emits chan(a), having taken a), every state q carries b(q) (the path is on a blank
 *   after arriving in q).  A value is (d, n, e): the fp64 acoustic sum, the number of characters, the entry frame (search only).
 *   Values are compared by key = d + bonus * (double) n (a product, then a sum: never fused) ; the largest wins, the earlier candidate
 *   on equality.  Frame t, from the values of frame t - 1:
 *     nb'(a): stay nb(a) ; b(src) ; the arcs x into src with chan(x) != chan(a), by ascending id ; in search, when src == 0, the fresh
 *       entry (0, 0, t).  d' = d + w(t, chan(a)), n' = n + 1 unless stay won, e' = e.
 *     b'(q): stay b(q) ; the arcs into q by ascending id.  d' = d + w(t, 0), n and e the winner's.
 *   One workgroup per span (decode) or line (search) on a grid of at most 2048 workgroups, sized by the automaton (64..1024 threads).
 *
 * Decode: the best string of the language over each span, plain max-product CTC with outer blanks.  w = lp[t,c] = ln(max((double)
 *   E[t,c], 1e-30)) ; before frame 0 everything is -inf except b(0) = (0, 0).  End candidates after the last frame: the arcs into
 *   accepting states by ascending id, then b(q) of accepting q ascending.
 *   spans [n,3] int32 on the DEVICE: (line, first frame, one past the last frame), clamped as dtlr_ctc_align clamps them: every line
 *     to [0, B), every frame to [0, T], every span to its first Tmax frames ; Tmax >= 0: the longest span, as the caller states it ;
 *   Lcap >= Tmax, else DTLR_ESHAPE.
 *   Outputs, every element written on every call: labels [n,Lcap] int32: the best string's channels, left-packed, padded with -1 ;
 *   length [n] int32: its characters, -1 when no string of the language fits the span ; score [n] fp64: d WITHOUT the bonus (-inf
 *   when length is -1) ; base [n] fp64: the sum over the span's frames, in frame order, of ln(max((double) max_c E[t,c], 1e-30)).
 *   A span of 0 frames: length 0 and score 0 when the start state accepts, else -1 and -inf ; base 0.
 *   workspace: dtlr_pattern_decode_workspace_bytes(n, n_states, n_arcs, Tmax) bytes, 16-byte aligned.  Per workgroup (G = min(n, 2048)
 *   of them), with N = n_arcs + n_states, rounded up to 16:
 *     24 N  two buffers of (d fp64, n int32) ; 8 (Tmax + 1) n_states  per frame (and once for the end) the two records of a state:
 *     the best arc into it and the best whose channel differs from the first's ; Tmax N  one byte per arc and frame (which candidate
 *     won) and per state and frame (whether b moved).
 *
 * Search: every occurrence of the language in every line, free start and end, no outer blanks, over all T frames.  w = g(t,c) =
 *   lp[t,c] - ln(max((double) max_c E[t,c], 1e-30)), exactly 0 where E[t,c] is the frame's fp32 maximum.  Everything starts at -inf ;
 *   a hit enters through the fresh entry and ends on the last frame of its last character.  r[t] = the best nb'(a) over the arcs into
 *   accepting states by key, lowest arc id on ties: (d[t], n[t], start[t]).  Frame t qualifies when d[t] is finite and d[t] >= n[t] *
 *   ln_min_conf (-inf allowed).  Hits: up to H (1..16, else DTLR_ESHAPE) qualifying frames by descending key, the smaller t on equal
 *   keys ; a frame whose [start[t], t] overlaps a hit already taken is skipped.  The automaton must not accept the empty string (the
 *   host refuses it).
 *   Outputs, every element written on every call: count [B] int32 ; start, end, nchar [B,H] int32 padded with -1 ; ratio [B,H] fp64
 *   (= d) padded with 0, in the order taken.
 *   workspace: dtlr_pattern_search_workspace_bytes(B, n_states, n_arcs, T) bytes, 16-byte aligned.  Per workgroup (G = min(B, 2048)),
 *   rounded up to 16: 32 N  two buffers of (d fp64, n int32, e int32) ; 8 n_states  the two records ; 24 T  r's d and key, n, start.
 * B == 0 or n == 0: nothing is done.  Asynchronous on `stream`; never synchronises. */
int dtlr_pattern_decode(const float *emissions, int B, int T, int V, const int *spans, int n, int Tmax,
                        const int *arc_src, const int *arc_chan, const int *dst_start, const int *accept, int n_states, int n_arcs,
                        double bonus, int *labels, int Lcap, int *length, double *score, double *base,
                        void *workspace, void *stream);
long dtlr_pattern_decode_workspace_bytes(int n, int n_states, int n_arcs, int Tmax);
int dtlr_pattern_search(const float *emissions, int B, int T, int V,
                        const int *arc_src, const int *arc_chan, const int *dst_start, const int *accept, int n_states, int n_arcs,
                        double bonus, double ln_min_conf, int H, int *count, int *start, int *end, double *ratio, int *nchar,
                        void *workspace, void *stream);
long dtlr_pattern_search_workspace_bytes(int B, int n_states, int n_arcs, int T);

#ifdef __cplusplus
}
#endif

#endif /* DTLR_PATTERN_H */

/* hyena_decode.h -- C ABI of the incremental Hyena operator step: one position per call, or a block of up to HYENA_DECODE_TMAX known
 * positions per call (the last section of this comment) (same library, libhyena_fftconv.so; kernels in
 * hyena_dna_amd/csrc/decode_kernels.h).
 *
 * Order 2, one head, one block, inner factor 1, short_filter_order 3 (the fused route of HyenaOperator).  One call of each entry point
 * advances ALL B sequences by one position t; t is read from device memory (`pos`, one int) by every kernel and advanced by
 * hyena_decode_post, so a captured graph of the three calls serves every position.  A position outside [0, Lcap) makes the kernels do
 * nothing (and the position stays where it is).
 *
 *   x    : in_proj output of position t WITHOUT its bias, element (c, b) at b ldx + c (ldx >= 3D), `dtype`
 *   bin  : (3D,) fp32 in_proj bias or NULL;  w : (3D, 3) fp32 short-filter taps;  b : (3D,) fp32 short-filter bias
 *   tail : (3D, Bcap, 2) fp32, the raw x of positions t - 2, t - 1 (what the prefill leaves; values before position 0 are not read)
 *   vg   : the history of the convolution's input v * x1, (Bcap, D, lda) `dtype`, row (b, d) at (b D + d) lda, lda >= Lcap, lda % 8 == 0,
 *          16-byte aligned; column t is written by hyena_decode_pre
 *   x0   : (B, D) fp32, the gate of position t (pre writes, post reads)
 *   k    : (D, ldk) fp32 filter (column j = tap j: HyenaFilter.filter_dl(Lcap)), ldk >= Lcap, ldk % 4 == 0, 16-byte aligned
 *   part : hyena_decode_partial_floats(B, D, Lcap) fp32 of scratch, [chunk][B][D] partial sums (no atomics: results are deterministic)
 *   fb   : (D,) fp32 filter bias or NULL;  z : (B, D) `dtype`, the out_proj operand of position t
 * 1 <= B <= Bcap, 1 <= Lcap <= 2^20.  Bad arguments return HYENA_ERR_BAD_ARG before anything is launched.  Asynchronous on `stream`.
 *
 * Per-row positions (hyena_decode_*_rows): the same three calls for a batch whose sequences stand at different positions.  `pos` points
 * at B ints in device memory, row b is advanced from t_b = pos[b]: hyena_decode_pre_rows writes column t_b of row b's history,
 * hyena_decode_conv_rows sums over s <= t_b (one partial per (chunk, b, d) with chunk * 8192 <= t_b; the other slots of `part` are neither
 * written nor read), hyena_decode_post_rows reads those partials and vg[b, d, t_b] and then advances pos[b] by one.  A row whose t_b is
 * outside [0, Lcap) is parked: its z row, history, tail and position stay as they are, the other rows advance.  History columns past t_b
 * of row b must hold finite values (they may be read and are multiplied by a zero tap).  All other arguments, their checks and the
 * stream semantics are those above; with all pos[b] equal the results equal the single-position entry points' bit for bit.
 *
 * Fan-out (hyena_decode_*_fan): the same three calls for G prompts that are each continued n = `fan` times.  B = G fan rows, row b belongs
 * to group b / fan, and all rows stand at the one position *pos.  Below S -- a multiple of 8192 (the history chunk), 0 <= S <= Lcap, in
 * practice (prompt length / 8192) 8192 -- the rows of a group have the same history, and it is kept once:
 *   vgs  : shared history (G, D, lds) `dtype`, columns [0, S) of group g in row (g D + d) lds; lds >= S, lds % 8 == 0, 16-byte aligned;
 *          read by hyena_decode_conv_fan only, may be NULL when S == 0
 *   vgr  : per-row history (Bcap, D, ldr) `dtype`, column t >= S of row b at index t - S of row (b D + d) ldr; ldr >= max(Lcap - S, 1),
 *          ldr % 8 == 0, 16-byte aligned; hyena_decode_pre_fan writes index t - S
 * hyena_decode_conv_fan computes the partial of a chunk below S once per group, into slot [chunk][g fan][d] of `part` (the layout and size
 * of hyena_decode_partial_floats(B, D, Lcap); the group's other slots of that chunk are neither written nor read), and one partial per
 * row for the chunks from S on; hyena_decode_post_fan sums row b's partials in chunk order, taking chunk < S / 8192 from slot g fan.  On
 * the batch whose B rows hold the replicated history the single-position entry points give the same z, x0, tail, history column and
 * position, bit for bit.  A position outside [S, Lcap) makes the kernels do nothing.  Bad arguments -- those above, and S not a multiple of
 * 8192, S > Lcap, fan < 1, B not a multiple of fan, a misaligned pointer or pitch -- return HYENA_ERR_BAD_ARG before anything is launched.
 *
 * Block step (hyena_decode_*_block, and *_block_fan for the fan-out layout): T known positions appended per call, 1 <= T <=
 * HYENA_DECODE_TMAX.  All B rows advance from t0 = *pos (device memory, read by every kernel) to t0 + T:
 *   x    : (B, T, 3D) `dtype`, the in_proj output of positions t0 ... t0 + T - 1 without bias, element (b, i, c) at (b T + i) ldx + c
 *   x0   : (B, T, D) fp32 and z : (B, T, D) `dtype`, element (b, i, d) at (b T + i) D + d
 *   part : hyena_decode_block_partial_floats(B, D, Lcap, T) fp32, [chunk][B][T][D]: part[chunk][b][i][d] = sum over the chunk's s <= t0 + i
 *          of k[d, t0 + i - s] vg[b, d, s].  A chunk that starts past t0 + i is not read for output i (a chunk that starts inside the
 *          block, t0 < chunk * 8192 <= t0 + T - 1, has its slots of the earlier outputs written with 0; chunks past t0 + T - 1 are not
 *          written at all); the fan form writes and reads a chunk below S in slot b = g fan only, as hyena_decode_conv_fan does.
 * hyena_decode_pre_block writes history columns t0 ... t0 + T - 1 and leaves positions t0 + T - 2, t0 + T - 1 in `tail`;
 * hyena_decode_conv_block streams every history segment ONCE for the T outputs (about the bytes of one single-position step);
 * hyena_decode_post_block writes z and then sets *pos = t0 + T (a second, one-thread launch on the same stream: the kernel that reads
 * the position runs on many workgroups).  After one block step, z, x0, the history columns, tail and pos equal what T calls of the
 * single-position entry points (the fan form: of the _fan entry points) leave, BIT FOR BIT, for the three dtypes: every output keeps
 * its summation order (csrc/decode_kernels.h).  The history columns up to t0 + T - 1 + 7 must hold finite values (they are read for the
 * block's earlier outputs against a zero tap).  If t0 < 0 (fan: t0 < S) or t0 + T > Lcap the kernels do nothing and the position stays.
 * Bad arguments -- T outside [1, HYENA_DECODE_TMAX] and everything the single-position and fan entry points refuse -- return
 * HYENA_ERR_BAD_ARG before anything is launched.  There is no block form of the per-row (_rows) step.
 *
 * Lookahead carry (hyena_decode_carry, hyena_decode_conv_la, hyena_decode_post_la; the plain cache only): the convolution is linear in the
 * history, so the share of the next W outputs that comes from the positions already cached is taken ahead, in ONE pass over the history,
 * and a step then reads only the columns written since.  1 <= W <= HYENA_DECODE_TMAX.
 *   carry : (B, W, D) fp32, element (b, j, d) at (b W + j) D + d;  base : one int in device memory, the position of the last refresh
 * hyena_decode_carry, with t0 = *pos: carry[b, j, d] = sum_{s < t0} k[d, t0 + j - s] vg[b, d, s] for 0 <= j < min(W, Lcap - t0) (the other
 * slots are not written), then *base = t0 (a one-thread launch behind the others).  `part` is hyena_decode_carry_partial_floats(B, D, Lcap,
 * W) fp32 of scratch, [chunk][B][W][D], written for the chunks that start below t0 and summed in chunk order; no atomics.  History columns
 * at and past t0 contribute exactly nothing whatever they hold (up to 7 of them are loaded); t0 = 0 gives exact zeros and reads no
 * history.  t0 outside [0, Lcap): nothing is written, *base stays.
 * hyena_decode_conv_la / hyena_decode_post_la are hyena_decode_conv / hyena_decode_post for a position t = *pos with lo = *base <= t < lo + W
 * (between them hyena_decode_pre is used as it is): conv_la sums over s in [lo, t] only -- part is 2 B D fp32, [x][B][D] for chunk
 * lo / 8192 + x, x = 1 written only if t has reached that chunk -- and post_la adds carry[b, t - lo, d], then the one or two partials in
 * chunk order, then does what hyena_decode_post does (fb, the rounding, the gate, *pos = t + 1).  Columns below lo inside the first loaded
 * vector and up to 7 past t meet a zero tap and must be finite.  With lo = 0 and a zero carry the results equal those of
 * hyena_decode_conv + hyena_decode_post bit for bit.  If t is outside [0, Lcap), lo is negative or t - lo is outside [0, W) both calls
 * write nothing and the position stays.  hyena_decode_pre knows nothing of the window and parks on t outside [0, Lcap) alone: issued at a
 * t in the cache but outside [lo, lo + W) it still writes history column t, shifts the tail and writes x0, while conv_la / post_la park
 * and *pos stays -- so the CALLER keeps lo <= t < lo + W (a hyena_decode_carry before the step whenever t = lo + W) or, where it issues
 * such a step knowingly (a graph warm-up), saves and restores the tail; column t is rewritten by the real step at t.  Bad arguments -- W outside [1, HYENA_DECODE_TMAX], a null carry or base, and everything the
 * single-position entry points refuse -- return HYENA_ERR_BAD_ARG before anything is launched. */
#ifndef HYENA_DECODE_H
#define HYENA_DECODE_H
#include <stddef.h>
#define HYENA_DECODE_TMAX 64
#ifdef __cplusplus
extern "C" {
#endif

size_t hyena_decode_partial_floats(int B, int D, int Lcap);
/* short conv of position t, vg[:, :, t] = x1c * vc, x0 = x0c, tail shifted */
int hyena_decode_pre(const void* x, int ldx, const float* bin, const float* w, const float* b, float* tail, void* vg, float* x0, const int* pos,
                     int B, int Bcap, int D, int Lcap, int lda, int dtype, void* stream);
/* part[chunk][b][d] = sum over the chunk's s <= t of k[d, t - s] vg[b, d, s] */
int hyena_decode_conv(const float* k, int ldk, const void* vg, float* part, const int* pos, int B, int D, int Lcap, int lda, int dtype,
                      void* stream);
/* z = round(round(sum_chunks part + fb vg_t) * x0); then *pos = t + 1 */
int hyena_decode_post(const float* part, const void* vg, const float* fb, const float* x0, void* z, int* pos, int B, int D, int Lcap, int lda,
                      int dtype, void* stream);

/* the three calls above with one position per row: pos points at B ints (see the header comment) */
int hyena_decode_pre_rows(const void* x, int ldx, const float* bin, const float* w, const float* b, float* tail, void* vg, float* x0,
                          const int* pos, int B, int Bcap, int D, int Lcap, int lda, int dtype, void* stream);
int hyena_decode_conv_rows(const float* k, int ldk, const void* vg, float* part, const int* pos, int B, int D, int Lcap, int lda, int dtype,
                           void* stream);
int hyena_decode_post_rows(const float* part, const void* vg, const float* fb, const float* x0, void* z, int* pos, int B, int D, int Lcap,
                           int lda, int dtype, void* stream);

/* the three calls above for B = G fan rows: history columns [0, S) once per group (vgs), [S, Lcap) per row (vgr) (see the header comment) */
int hyena_decode_pre_fan(const void* x, int ldx, const float* bin, const float* w, const float* b, float* tail, void* vgr, float* x0,
                         const int* pos, int B, int Bcap, int D, int Lcap, int S, int ldr, int dtype, void* stream);
int hyena_decode_conv_fan(const float* k, int ldk, const void* vgs, const void* vgr, float* part, const int* pos, int B, int fan, int D,
                          int Lcap, int S, int lds, int ldr, int dtype, void* stream);
int hyena_decode_post_fan(const float* part, const void* vgr, const float* fb, const float* x0, void* z, int* pos, int B, int fan, int D,
                          int Lcap, int S, int ldr, int dtype, void* stream);

/* the block step: T positions per call (see the header comment); x (B, T, 3D), x0 and z (B, T, D), part [chunk][B][T][D] */
size_t hyena_decode_block_partial_floats(int B, int D, int Lcap, int T);
int hyena_decode_pre_block(const void* x, int ldx, const float* bin, const float* w, const float* b, float* tail, void* vg, float* x0,
                           const int* pos, int B, int Bcap, int D, int Lcap, int lda, int T, int dtype, void* stream);
int hyena_decode_conv_block(const float* k, int ldk, const void* vg, float* part, const int* pos, int B, int D, int Lcap, int lda, int T,
                            int dtype, void* stream);
int hyena_decode_post_block(const float* part, const void* vg, const float* fb, const float* x0, void* z, int* pos, int B, int D, int Lcap,
                            int lda, int T, int dtype, void* stream);
int hyena_decode_pre_block_fan(const void* x, int ldx, const float* bin, const float* w, const float* b, float* tail, void* vgr, float* x0,
                               const int* pos, int B, int Bcap, int D, int Lcap, int S, int ldr, int T, int dtype, void* stream);
int hyena_decode_conv_block_fan(const float* k, int ldk, const void* vgs, const void* vgr, float* part, const int* pos, int B, int fan, int D,
                                int Lcap, int S, int lds, int ldr, int T, int dtype, void* stream);
int hyena_decode_post_block_fan(const float* part, const void* vgr, const float* fb, const float* x0, void* z, int* pos, int B, int fan, int D,
                                int Lcap, int S, int ldr, int T, int dtype, void* stream);

/* the lookahead carry (see the header comment): carry (B, W, D) fp32, base one device int; part of conv_la / post_la is 2 B D fp32 */
size_t hyena_decode_carry_partial_floats(int B, int D, int Lcap, int W);
int hyena_decode_carry(const float* k, int ldk, const void* vg, float* part, float* carry, const int* pos, int* base, int B, int D, int Lcap,
                       int lda, int W, int dtype, void* stream);
int hyena_decode_conv_la(const float* k, int ldk, const void* vg, float* part, const int* pos, const int* base, int B, int D, int Lcap, int lda,
                         int W, int dtype, void* stream);
int hyena_decode_post_la(const float* part, const float* carry, const void* vg, const float* fb, const float* x0, void* z, int* pos,
                         const int* base, int B, int D, int Lcap, int lda, int W, int dtype, void* stream);

/* Token sampling, the last node of the per-token graph: one wavefront per row of `logits` (B, V) `dtype`, row b at b ldl, 1 <= Vlive <= V <= 64
 * (columns >= Vlive, the padded vocabulary, are never chosen).  Row b stands at column c = col[b] of `seq` (B, ncols) int64, row b at b lds:
 *   c outside [0, ncols): parked, nothing of the row is read or written;  done[b] != 0: next[b ldn] = pad and nothing else;  otherwise
 *   scores[b, c, i] = l_i / T for i < V (scores (B, ncols, V) fp32 or NULL; T = max(temperature, 1e-6)), the token is drawn, and
 *   seq[b, c] = next[b ldn] = tok, col[b] = c + 1, done[b] = 1 if tok == eos (eos < 0: none).
 * The draw is a total function of the logits.  Rank r_i = #{ j < Vlive : j comes before i }, where a NaN comes before every number and, among
 * NaNs, the lower index first; among numbers j comes before i iff l_j > l_i, or l_j == l_i and j < i.  That is the order of
 * torch.sort(l, descending=True, stable=True), and the ranks are a permutation of 0 .. Vlive - 1 for every input.  top_k <= 1 takes rank 0
 * (torch.argmax: the first NaN, else the maximum, lowest index on a tie; top_p and the seed do not matter).  A row whose rank-0 live logit is
 * not finite -- a NaN, a +inf, or -inf, which means every live logit is -inf -- emits its rank-0 token whatever top_k, top_p and T are; u is
 * drawn and reported, and col, done, eos, pad and scores (l / T verbatim, the NaN included) behave as for any other row.  Otherwise keep r_i < min(top_k, Vlive), p_i = exp((l_i - max l) / T) in fp32 over them and Z their sum;
 * keep token i iff the kept mass ranked strictly before it is < top_p Z (0 < top_p <= 1); with u = (w >> 8) 2^-24, w word 0 of
 * Philox4x32-10(counter (c, b, 0, 0), key *seed (low, high word)), the token is the kept one of smallest rank whose inclusive cumulative
 * mass exceeds u Z' (Z' the kept mass), else the last kept one.  u_out (B,) fp32 or NULL receives u.  `seed` is a DEVICE pointer to one
 * 64-bit word.  The emitted token is always in [0, Vlive).  Bad arguments (a null required pointer, V > 64, Vlive
 * outside [1, V], top_p outside (0, 1], an unknown dtype, ldl < V, lds < ncols) return HYENA_ERR_BAD_ARG before anything is launched. */
int hyena_decode_sample(const void* logits, long ldl, int dtype, int B, int V, int Vlive, float temperature, int top_k, float top_p,
                        const unsigned long long* seed, int eos, int pad, int* col, int* done, long long* seq, long lds, int ncols,
                        long long* next, long ldn, float* scores, float* u_out, void* stream);

/* Constrained token sampling with token log-probs: hyena_decode_sample (every argument and rule above) with an allowed set per row and
 * new-token number.  `start` (B,) int32 is the column of row b's first new token (the prompt length; lengths[b] for ragged prompts), and
 * n = col[b] - start[b] the number of the token the row draws now.  `allow`: 64-bit masks, row b's mask for its n-th new token at
 * allow[b lda + n], n < nallow; lda = 0: one row of masks for the whole batch; bit v set: token v may be emitted.  The allowed set is
 *   A = { v < Vlive : bit v of the mask };  A = the whole live vocabulary where allow is NULL, n lies outside [0, nallow), or the mask has
 *   no bit below Vlive (the kernel ends a captured graph and cannot raise: it stays a total function).
 * Every rule of hyena_decode_sample then reads "A" where it reads "the live tokens": ranks are taken among A (a NaN first, then numbers by
 * value, then by index), top_k <= 1 takes rank 0 of A, k = min(top_k, |A|), p_i = exp((l_i - max_A l) / T) summed in rank order, the nucleus
 * is a prefix of that order, the draw is the same Philox word of (seed, row, column), and a row whose rank-0 logit within A is not finite
 * emits that token.  eos ends a row when it is emitted, hence only where A holds it.  Parked and done rows behave as above; a done row
 * writes next = pad and nothing else, its log-prob slot included.  (col[b], done[b] and start[b] are read for every row, together; a parked
 * or done row's logits and masks are not.)  The emitted token is always in A.
 * `logprobs` (row b at b ldp, fp32) or NULL: logprobs[b ldp + n] = (l_tok - m) - log(sum_{j < Vlive} exp(l_j - m)), m = max_{j < Vlive} l_j
 * -- the model's own distribution over ALL live tokens at temperature 1, not the constrained or tempered one -- in fp32, the sum taken
 * serially in index order (a pure function of the row's logits).  Where m or the sum is not finite (a live NaN or +inf, or every live logit
 * -inf) the slot receives NaN; a token whose own logit is -inf among finite ones gets -inf.  Written only for n in [0, ldp).
 * With allow == NULL and logprobs == NULL, or with every mask all ones, seq, next, col, done, scores and u_out equal hyena_decode_sample's
 * bit for bit.  Bad arguments as for hyena_decode_sample, and: start == NULL with allow or logprobs given, nallow < 1 or 0 < lda < nallow
 * with allow given, ldp < 1 with logprobs given. */
int hyena_decode_sample_constrained(const void* logits, long ldl, int dtype, int B, int V, int Vlive, float temperature, int top_k, float top_p,
                                    const unsigned long long* seed, int eos, int pad, int* col, int* done, long long* seq, long lds,
                                    int ncols, long long* next, long ldn, float* scores, float* u_out, const unsigned long long* allow,
                                    long lda, int nallow, const int* start, float* logprobs, long ldp, void* stream);

/* Beam search over the fan-out layout: the k = `fan` beams of a prompt are the k rows of a fan group, row g k + r holding rank r of prompt
 * g, best first.  1 <= k <= HYENA_DECODE_BEAM_MAX, B = G k rows, 1 <= Vlive <= V <= 64.
 *
 * hyena_decode_beam -- the beam step, in the sampler's place as the last node of a step: one 64-lane workgroup per group.  Group g stands at
 * column c = col[g k] (one value per group); c outside [0, ncols): parked, nothing of the group is read or written.  Otherwise
 *   1. log-probabilities.  For a live row j (done[j] == 0), lp[j][i] = (l_i - m) - log(sum_{v < Vlive} exp(l_v - m)), m the maximum of the
 *      live logits (NaNs skipped): exactly the value hyena_decode_sample_constrained defines for its `logprobs` -- fp32, the sum serial in
 *      index order, NaN where m or the sum is not finite.  The model's own distribution at temperature 1 over ALL live tokens, not
 *      renormalised over the allowed set: a beam's score is the log-likelihood of its tokens under the model.
 *   2. candidates.  A live row j contributes every token i of its allowed set A -- `allow`, `lda`, `nallow`, `start` and the rule that an
 *      empty set means the whole live vocabulary as in hyena_decode_sample_constrained, n = c - start[row] -- with score
 *      beam_score[j] + lp[j][i].  A finished row contributes exactly ONE candidate: token `pad`, its score unchanged (flat index j V).
 *      Everything else is excluded.  Every row yields a candidate, so at least k exist.
 *   3. selection.  The first k candidates in this order: numbers by score descending (-inf included), then NaN scores; ties -- equal
 *      scores, two NaNs -- by the flat index j V + i ascending.  The order is total for every input.  Rank r goes to row g k + r.
 *   4. writes for row b = g k + r: parent[b] = the ABSOLUTE row index of the candidate's row; beam_score[b] = its score; done[b] = the
 *      parent's flag, or 1 if the token is `eos` (eos < 0: none); next[b ldn] = the token (`pad` for a finished row); col[b] = c + 1; and
 *      the records tok_hist / parent_hist / lp_hist [b ldh + n] = token / parent / lp of the token (0 for a finished row's pad), n =
 *      c - start[b], written only for n in [0, nrec) (each record may be NULL).  One lane writes, after every lane has read the group's
 *      state; no atomics.
 * The caller initialises beam_score to 0 for rank 0 and -inf for the other rows of every group: the first step's k identical rows then
 * expand as one.  Bad arguments (a null required pointer -- everything but allow and the records --, fan outside [1, HYENA_DECODE_BEAM_MAX],
 * B not a multiple of fan, V > 64, Vlive outside [1, V], an unknown dtype, ldl < V, ncols < 1, ldn < 1, nallow < 1 or 0 < lda < nallow
 * with allow given, nrec < 1 or ldh < nrec with a record given) return HYENA_ERR_BAD_ARG before anything is launched.
 *
 * hyena_decode_reorder_fan -- re-parents the rows of ONE layer's fan-out cache in place (what a key-value cache calls _reorder_cache).  With
 * t1 = *pos (the position hyena_decode_post_fan left) and c0 the first column that can differ between the rows of a group (the prompt
 * length), S <= c0 <= Lcap:
 *     vgr[b, d, s - S] = old vgr[parent[b], d, s - S]   for c0 <= s < t1, every d;      tail[c, b, :] = old tail[c, parent[b], :]   for c < 3 D
 * for every row b < B.  A parent[b] outside b's own group is taken as b.  t1 outside [S, Lcap]: nothing is written.  The shared history,
 * the columns below c0 and the columns from t1 on are never touched.  One thread owns one (group, channel, column) -- or (group, tail
 * element) -- for all k rows, loads the k values through parent[] and only then stores them: no scratch, no second launch.  The grid
 * depends on Lcap - c0, the live range on *pos: one captured launch serves every token.
 * Bytes moved per layer and step: 2 B D (t1 - c0) sizeof(dtype) for the history (read + write) plus 48 B D for the tails -- linear in the
 * number of tokens generated so far and independent of the prompt length.
 * Bad arguments (everything hyena_decode_post_fan refuses for vgr / B / fan / D / Lcap / S / ldr / dtype, a null tail, parent or pos,
 * fan > HYENA_DECODE_BEAM_MAX, Bcap < B, c0 outside [S, Lcap]) return HYENA_ERR_BAD_ARG before anything is launched.
 *
 * hyena_decode_beam_backtrack -- once after the last step, one thread per returned row q = g n_ret + r (1 <= n_ret <= fan): starting at row
 * g k + r it walks the records from step n_done - 1 back to step 0: seq[q lds + P + i] = tok_hist[row, i], logprobs[q ldp + i] =
 * lp_hist[row, i] (logprobs may be NULL), then row = parent_hist[row, i] (a parent outside [0, B) is taken as the row itself).
 * 0 <= n_done <= ldh, lds >= P + n_done, ldp >= n_done; bad arguments return HYENA_ERR_BAD_ARG. */
#define HYENA_DECODE_BEAM_MAX 16
int hyena_decode_beam(const void* logits, long ldl, int dtype, int B, int fan, int V, int Vlive, int eos, int pad, int* col, int* done,
                      float* beam_score, const int* start, int* parent, long long* next, long ldn, int ncols,
                      const unsigned long long* allow, long lda, int nallow, int* tok_hist, int* parent_hist, float* lp_hist, long ldh,
                      int nrec, void* stream);
int hyena_decode_reorder_fan(void* vgr, float* tail, const int* parent, const int* pos, int B, int Bcap, int fan, int D, int Lcap, int S,
                             int c0, int ldr, int dtype, void* stream);
int hyena_decode_beam_backtrack(const int* tok_hist, const int* parent_hist, const float* lp_hist, long ldh, int B, int fan, int n_done,
                                int n_ret, long long* seq, long lds, int P, float* logprobs, long ldp, void* stream);

/* Automaton-constrained generation: the allowed set of a row depends on the tokens the row itself has emitted, through the state of a
 * deterministic automaton over the token alphabet that the row carries in device memory.
 *   delta  (S, V) int32, V the number of logit columns: delta[s V + v] is the state after token v in state s, -1 where v is forbidden there;
 *   M      (Nt, S) 64-bit masks: bit v of M[n S + s] says that token v may be the row's n-th new token in state s -- the host computes it
 *          backwards from the end (an accepting state after the last token, positional masks, eos and min_new_tokens folded in), so a row
 *          that follows M can always be completed to a word of the language.  Nt == 1: nothing depends on n, row 0 serves every token;
 *   dstate (B,) int32: the state of every row, initialised by the caller (the automaton run over the end of the prompt).
 * 1 <= S <= HYENA_DECODE_AUTOMATON_MAX_STATES, Nt >= 1, Nt S <= HYENA_DECODE_AUTOMATON_MAX_TABLE.
 *
 * hyena_decode_sample_automaton -- hyena_decode_sample_constrained with the row's mask M[(Nt == 1 ? 0 : n) S + s], s = dstate[b],
 * n = col[b] - start[b].  Everything after the mask is that function operation for operation: A (a mask with no bit below Vlive: the
 * whole live vocabulary), ranks among A, greedy, top-k, top-p, the Philox word of (seed, row, column), eos, pad, scores, u_out and the
 * log-prob over all live tokens.  After the token is chosen dstate[b] = delta[s V + tok].  The state is left as it is for a finished row,
 * for a row that has just emitted eos, for a -1 transition (reachable only through the whole-vocabulary fall-back) and for an s outside
 * [0, S); such a row, and with Nt > 1 a row whose n lies outside [0, Nt), samples unmasked.  Parked rows touch nothing.  With S = 1,
 * delta == 0 and M one row of masks the results equal hyena_decode_sample_constrained's with allow = M, lda = 0, bit for bit.
 * Bad arguments as for hyena_decode_sample_constrained, and: a null M, delta, dstate or start, S or Nt S out of range, Vdelta (the number of
 * columns of delta) != V -- HYENA_ERR_BAD_ARG before anything is launched.
 *
 * hyena_decode_beam_automaton -- hyena_decode_beam with row j's allowed set M[(Nt == 1 ? 0 : n) S + dstate[row j]] (the same fall-backs).
 * All k states of a group are read before any of its rows is written.  Rank r, which continues row p with token tok, receives
 * dstate = delta[dstate_old[p] V + tok]; the parent's state as it is for a finished beam's pad candidate, for eos, for a -1 transition and
 * for a state outside [0, S).  The order, the selection and the records are hyena_decode_beam's; hyena_decode_reorder_fan is not involved
 * (the state travels inside this kernel).  Bad arguments as for hyena_decode_beam and as above. */
#define HYENA_DECODE_AUTOMATON_MAX_STATES 4096
#define HYENA_DECODE_AUTOMATON_MAX_TABLE (1L << 22)
int hyena_decode_sample_automaton(const void* logits, long ldl, int dtype, int B, int V, int Vlive, float temperature, int top_k, float top_p,
                                  const unsigned long long* seed, int eos, int pad, int* col, int* done, long long* seq, long lds, int ncols,
                                  long long* next, long ldn, float* scores, float* u_out, const unsigned long long* M, int Nt, int S,
                                  const int* delta, int Vdelta, int* dstate, const int* start, float* logprobs, long ldp, void* stream);
int hyena_decode_beam_automaton(const void* logits, long ldl, int dtype, int B, int fan, int V, int Vlive, int eos, int pad, int* col,
                                int* done, float* beam_score, const int* start, int* parent, long long* next, long ldn, int ncols,
                                const unsigned long long* M, int Nt, int S, const int* delta, int Vdelta, int* dstate, int* tok_hist,
                                int* parent_hist, float* lp_hist, long ldh, int nrec, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HYENA_DECODE_H */

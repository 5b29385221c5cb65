/* libwct_hip -- seeded style variations: the part of the C ABI behind `--diversity`.
 *
 * For one content and one style the cascade has exactly one result.  The colouring step of whitening / colouring, however, needs only
 * SOME square root of the style covariance: T = S Z cov_c^(-1/2) with any orthogonal Z reaches the same target covariance as
 * T = S cov_c^(-1/2), because S Z Z^T S^T = cov_s, but through a different map (Wang et al., "Diversified Arbitrary Style Transfer via
 * Deep Feature Perturbation", CVPR 2020).  Different Z give visibly different stylisations with identical feature statistics.  This
 * header makes a seeded Z and post-multiplies prepared style slots by it.  Everything in wct_hip.h holds here too: return codes,
 * wct_last_error, device pointers, one context = one stream, asynchronous calls.
 *
 * The rotation Z(C, seed, stream_id, tag, strength), C even, 2..512, row-major fp64
 *
 *   generator   Philox4x32-10 exactly as wct_noise_uniform uses it (multipliers 0xD2511F53, 0xCD9E8D57, Weyl increments 0x9E3779B9,
 *               0xBB67AE85): key (seed & 0xffffffff, seed >> 32); counter of block i (i & 0xffffffff, i >> 32, stream_id,
 *               0x524F5400 | tag), tag in 0..255.  The noise image has 0 in that last word, so the two never share a stream.
 *   elements    element e = r C + c of a C x C matrix G is word e & 3 of block e >> 2, read as g = (double)(int32_t)word * 2^-31 (exact)
 *   scale       s = strength / (2.0 * sqrt(2.0 * C / 3.0)), in IEEE double, in that order.  It puts the spectral radius of A / strength
 *               just under 1 (0.59 at C = 8; 0.90 / 0.94 / 0.97 / 0.98 at C = 24 / 64 / 128 / 512)
 *   skew        r < c: A[r][c] = s * (g_rc - g_cr) -- the difference is exact, so there is one rounding --, A[c][r] = 0 - A[r][c],
 *               A[r][r] = 0: A is skew-symmetric bit for bit
 *   result      Z = (I - A)(I + A)^(-1), the Cayley transform of A: orthogonal for every A
 *
 * Z is a continuous family from Z = I at strength 0; its rotation angles 2 atan(strength mu_k) (+- i mu_k: the eigenvalues of
 * A / strength) reach about 90 degrees at strength 1 and about 165 degrees at WCT_DIVERSE_MAX_STRENGTH.
 *
 * Arithmetic: fp64 on the fp64 matrix cores, fixed summation orders.  B = I - A A (symmetric positive definite, eigenvalues in
 * [1, 1 + strength^2]) is formed symmetric bit for bit; R = B^(-1/2) runs through the solver of wct_solve; U = (I - A) R is orthogonal
 * and Z = U U.  Two exact rules: strength exactly 0 writes the identity exactly, with no solver; and the same five arguments give the
 * same bits on every call, in every context, whatever modules it has loaded and whatever it ran before.
 *
 * Only the wct transform can be diversified.  The optimal-transport map between two Gaussians is unique, AdaIN reads only the row
 * norms of S, which Z does not change, and the ot arithmetic assumes a symmetric S.  So the context keeps a per-level "rotated" mark:
 * wct_style_diversify sets it, whatever rewrites the slot clears it, and switching the context to ot or adain is WCT_ERR_STATE while
 * any mark is set.  A rotated slot travels through wct_style_export like any other; importing rotated statistics into another context
 * (whose mark stays clear) and reading them under ot or adain there is the caller's business.
 */
#ifndef WCT_HIP_DIVERSE_H
#define WCT_HIP_DIVERSE_H

#include "wct_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WCT_DIVERSE_MAX_STRENGTH 8

/* Z [C*C] (device fp64, row-major) as defined above; skew [C*C] (device fp64, or NULL) receives A.  C even, 2..512; tag 0..255;
 * strength in [0, WCT_DIVERSE_MAX_STRENGTH] -- negative, NaN or larger is WCT_ERR_INVALID, as is every other bad argument (a NULL Z, Z
 * overlapping skew), before anything is written.  Needs no loaded module and reads no state of the context.  On the caller's stream;
 * C > 128 synchronises it once (the solver's outcome check). */
int wct_rotation_make(wct_ctx* ctx, int C, uint64_t seed, uint32_t stream_id, unsigned tag, double strength, double* Z, double* skew);

/* For every level L in level_mask (bit L, levels 1..5), in place: F <- F Z(C_L, seed, stream_id, tag = L, strength), F = the
 * cov_s^(1/2) part of the level's prepared style slot; mu_s is untouched.  Then the slot's style-side fold is redone, exactly as
 * wct_style_import ends.  On the caller's stream, behind whatever prepared the slot.  Every entry that reads prepared statistics
 * (wct_stylize_prepared, wct_content_solve, wct_synthesize without a texture, wct_stylize_clip, wct_style_export, ...) then reads the
 * diversified slot without knowing it; a clip diversified once uses the same rotation for every frame.
 * Refusals, all before anything is written: a non-wct transform of the context, an empty mask, a bit outside levels 1..5 or a bad
 * strength is WCT_ERR_INVALID; a masked level without a loaded encoder or a prepared slot is WCT_ERR_STATE.
 * Strength exactly 0 leaves the slots untouched bit for bit (and sets no mark).
 * Calling it twice COMPOSES the two rotations (F Z1 Z2).  Anything that rewrites a slot resets it to that call's own statistics:
 * wct_style_prepare, wct_style_import, wct_style_blend, wct_stylize_interp, wct_stylize, wct_synthesize with a texture, ...
 * Workspace: allocated on the first call of a width and not after; NOT part of wct_reserve / wct_workspace_bytes, whose numbers do
 * not move. */
int wct_style_diversify(wct_ctx* ctx, unsigned level_mask, double strength, uint64_t seed, uint32_t stream_id);

/* wct_style_prepare + wct_style_diversify + wct_stylize_prepared in one call, bit-identical to those three public calls; every
 * refusal of wct_style_diversify that does not depend on prepared state comes before anything is written. */
int wct_stylize_diverse(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, unsigned level_mask, double strength,
                        uint64_t seed, uint32_t stream_id, float alpha, int num_run, float* out, int* Ho, int* Wo);

#ifdef __cplusplus
}
#endif
#endif /* WCT_HIP_DIVERSE_H */

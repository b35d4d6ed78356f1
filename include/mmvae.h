/* mmvae.h -- C ABI of the MI355X-native conv-VAE train path (libmmvae_hip.so).
 *
 * The reference (praateekmahajan/moving-mnist-vae) is pure Python and has no FFI of its own: the
 * arithmetic of its hot path is reached through torch.nn / torch.optim.  This header is therefore the
 * boundary a maintainer would bind (ctypes) in place of those calls.  Each entry point
 * cites the reference lines whose arithmetic it replaces (paths relative to the reference repository).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless marked "host"; nothing is allocated
 *     or freed by the library except the opaque mmvae_net handle (host memory only);
 *   - all calls are asynchronous on `stream` (a hipStream_t passed as void*), never synchronise, and are
 *     hipGraph-capturable;
 *   - return value: 0 (or a positive count where documented) on success, negative MMVAE_ERR_* on failure,
 *     with a human-readable message from mmvae_last_error();
 *   - dtype: 0 = f32 storage / exact-f32 MFMA, 1 = bf16 storage / bf16 MFMA with f32 accumulation.
 *     Parameters, gradients, BN statistics, latents and the reconstruction are always f32.
 *   - activation layout is NHWC; the network boundary (image in, reconstruction out) is NCHW like the
 *     reference (identical for the 1-channel image).
 */
#ifndef MMVAE_H_
#define MMVAE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define MMVAE_API __attribute__((visibility("default")))
#else
#define MMVAE_API
#endif

#define MMVAE_OK 0
#define MMVAE_ERR_ARG (-1)
#define MMVAE_ERR_HIP (-2)
#define MMVAE_ERR_WORKSPACE (-3)
#define MMVAE_ERR_UNSUPPORTED (-4)

#define MMVAE_F32 0
#define MMVAE_BF16 1
#define MMVAE_FP8 2     /* network handle only (BASELINE configs[4]): bf16 storage, but the forward convolutions of the deep layers (channel
                           counts that are multiples of 64, every one followed by a BatchNorm) run on v_mfma_f32_16x16x32_fp8_fp8: OCP e4m3
                           weights (static power-of-two scale per layer, absorbed exactly by the BatchNorm) x e4m3 activations (quantised
                           behind the fused BN+ReLU), f32 accumulation and statistics; the backward pass stays bf16 (straight-through).
                           Where the 64x64 last up-block runs on the stream kernels its two branch outputs (the largest tensors of the
                           step) are STORED as e4m3 bytes with a static scale of 16 the BatchNorms behind absorb */

/* Version of this header's signatures.  2: mmvae_conv2d_wgrad gained the caller-owned `scratch` argument (before `stream`);
 * 3: mmvae_convT_bwd_fused gained `dw2`, the weight-gradient entry points REQUIRE the scratch (partial images, fixed-order reduce: no
 * float atomics), new entries (stage_labels, encoder_fwd_staged, decoder_bwd_gauss, upblock / conv1x1_bwd_fused, set_sync_bn_comm2,
 * pixelcnn_*); in_channels 1..4.  A binding built against another version must not call this one (check mmvae_abi_version() ==
 * MMVAE_ABI_VERSION at load time). */
#define MMVAE_ABI_VERSION 3
MMVAE_API int mmvae_abi_version(void);
MMVAE_API const char* mmvae_last_error(void);          /* host string, valid until the next failing call on this thread */

/* ------------------------------------------------------------------ network handle
 * Describes VAE(in_channels, ., decoder_out_channels, ., z_dimension, pixelcnn=False, only_pixelcnn=False, ...,
 * require_rsample, ., input_image_size)  -- model.py:258-310 (encoder :88-112, decoder :153-179).  */
typedef struct mmvae_net mmvae_net;
MMVAE_API int mmvae_net_create(mmvae_net** out, int in_channels, int z_dimension, int out_channels, int image_size,
                     int need_logvar, int dtype);
/* Deeper-than-reference variant (BASELINE configs[3]): blocks_per_stage residual blocks in every encoder stage (_make_layer with
 * blocks > 1, model.py:132-146: the extra BasicBlocks keep the shape and have an identity shortcut) and in every decoder stage
 * (_make_up_block with num_layer > 1, model.py:196-209: the extra blocks come first; the reference's own extra DeconvBottleneck
 * cannot run -- 2x main path against an identity shortcut, :205-206 -- so here it is conv1x1 -> BN -> ReLU -> conv3x3 -> BN, +
 * identity, ReLU).  blocks_per_stage = 1 is the reference network. */
MMVAE_API int mmvae_net_create_ex(mmvae_net** out, int in_channels, int z_dimension, int out_channels, int image_size,
                        int need_logvar, int dtype, int blocks_per_stage);
MMVAE_API void mmvae_net_destroy(mmvae_net* net);
/* Flat storage sizes: f32 parameters, f32 BN running statistics, int64 num_batches_tracked counters; first
 * decoder parameter (for gradient bucketing); decoder output side (32 or 64, model.py:169,191). */
MMVAE_API int mmvae_net_sizes(const mmvae_net* net, int64_t* n_params, int64_t* n_bn_f32, int32_t* n_bn_i64,
                    int64_t* decoder_param_offset, int32_t* decoder_side);
/* state_dict inventory in the reference's registration order (183 entries at the default config).
 * kind: 0 parameter (offset into the flat parameter buffer), 1 BN f32 buffer, 2 BN int64 counter. */
MMVAE_API int mmvae_net_num_entries(const mmvae_net* net);
MMVAE_API int mmvae_net_entry(const mmvae_net* net, int index, char* name, int name_cap, int32_t* ndim, int32_t shape[4],
                    int32_t* kind, int64_t* offset);
/* Bytes of activation workspace needed for a batch of N frames (forward + backward). */
MMVAE_API size_t mmvae_net_workspace_bytes(mmvae_net* net, int N);

/* VAE_Encoder.forward, model.py:114-130 (BasicBlock.forward :39-55).  x: [N,1,S,S] f32.  Writes mu, logvar
 * [N,z] f32 (logvar may be NULL when need_logvar=0).  training!=0: batch statistics, running-stat update with
 * momentum 0.1 / unbiased variance and num_batches_tracked += 1 (nn.BatchNorm2d); else running statistics. */
MMVAE_API int mmvae_encoder_fwd(mmvae_net* net, int N, const float* x, const float* params, float* bn_f32, int64_t* bn_i64,
                      void* workspace, size_t workspace_bytes, float* mu, float* logvar, int training, void* stream);
/* Input staging (reference main.py:383-387, image = (label - mean) / std): labels (int64 as the reference's loader yields them,
 * label_bytes = 8, or uint8, label_bytes = 1; N * in_channels * S * S of them) -> `image` f32 [N,in_channels,S,S] (the caller's tensor:
 * network input and Gaussian-loss target) AND the storage-type copy in the workspace's input slot, in ONE pass.
 * mmvae_encoder_fwd_staged is mmvae_encoder_fwd for exactly that `image` right after: it skips the conversion pass over x (the caller
 * guarantees x has not changed since it was staged into this workspace). */
MMVAE_API int mmvae_net_stage_labels(mmvae_net* net, int N, const void* labels, int label_bytes, float mean, float stdv, float* image,
                           void* workspace, size_t workspace_bytes, void* stream);
MMVAE_API int mmvae_encoder_fwd_staged(mmvae_net* net, int N, const float* x, const float* params, float* bn_f32, int64_t* bn_i64,
                             void* workspace, size_t workspace_bytes, float* mu, float* logvar, int training, void* stream);
/* autograd of the above (loss.backward(), main.py:398): accumulates (+=) parameter gradients into `grads`
 * (same flat layout as params; caller zeroes).  No gradient is produced for the image. */
MMVAE_API int mmvae_encoder_bwd(mmvae_net* net, int N, const float* d_mu, const float* d_logvar, const float* params, float* grads,
                      void* workspace, size_t workspace_bytes, void* stream);
/* VAE_Decoder.forward, model.py:181-194 (DeconvBottleneck.forward :70-85).  encoding: [N,z] f32.
 * recon: [N,out_channels,Sd,Sd] f32 NCHW, Sd = decoder_side (crop by `adjust`, model.py:328-329, is the caller's view). */
MMVAE_API int mmvae_decoder_fwd(mmvae_net* net, int N, const float* encoding, const float* params, float* bn_f32, int64_t* bn_i64,
                      void* workspace, size_t workspace_bytes, float* recon, int training, void* stream);
MMVAE_API int mmvae_decoder_bwd(mmvae_net* net, int N, const float* d_recon, const float* params, float* grads, void* workspace,
                      size_t workspace_bytes, float* d_encoding /* may be NULL */, void* stream);
/* The same with the Gaussian reconstruction loss folded in (reference model.py:403, VAE.loss with decoder_out_channels == in_channels):
 * the gradient entering the decoder is d_recon = coef / sigma^2 * gscale[0] * (recon - target), recon being the reconstruction the last
 * mmvae_decoder_fwd on this workspace returned (full size, before any crop).  It is evaluated inside the output BatchNorm's backward
 * from the saved conv output and `target` [N,out_ch,S,S] f32 -- no d_recon tensor, two passes over the plane instead of four.
 * gscale: device scalar (the upstream gradient of the loss), nullable (= 1). */
MMVAE_API int mmvae_decoder_bwd_gauss(mmvae_net* net, int N, const float* target, float sigma, float coef, const float* gscale, const float* params,
                            float* grads, void* workspace, size_t workspace_bytes, float* d_enc, void* stream);

/* Weight gradients run on a side stream owned by the net.  By default every backward entry point orders
 * them before `stream` again when it returns.  mmvae_net_defer_join(net, 1): mmvae_decoder_bwd leaves its weight gradients in
 * flight; they are ordered before `stream` by the next mmvae_encoder_bwd on this net or by mmvae_net_join(net, stream), whichever
 * comes first -- call one of them before anything on `stream` reads the decoder's gradients (optimizer, all-reduce). */
MMVAE_API int mmvae_net_defer_join(mmvae_net* net, int enable);
MMVAE_API int mmvae_net_join(mmvae_net* net, void* stream);
/* The net's side stream, ordered behind everything enqueued on `stream` so far (`stream` itself when the net has none).  Work the caller
 * enqueues on it runs beside `stream` and is ordered before `stream` again by mmvae_net_join or the next backward entry point that joins
 * (above).  Used by the host side to take the loss scalars of reference model.py:385-406 (KL, MMD, NLL sums: logged values that no
 * gradient kernel reads) off the critical stream of a train step. */
MMVAE_API void* mmvae_net_fork(mmvae_net* net, void* stream);
/* The side stream itself (NULL when the net runs on one stream), without a new ordering edge: for work that only depends on what the
 * stream's earlier forks already ordered it behind (the host side enqueues the step's loss scalars there from the decoder's backward). */
MMVAE_API void* mmvae_net_side_stream(mmvae_net* net);
/* Backward form of the up-blocks on 16-wide maps (decoder.uplayer4; reference model.py:70-85 autograd).  1 (default): the block above hands
 * its input gradient down already masked by this block's join ReLU, the join BatchNorms' backward reduce runs unmasked and dy is evaluated
 * by the loaders of the two fused ConvTranspose2d backward passes -- no apply pass, no dy tensors.  0: reduce -> apply -> consumers, the form
 * every other block uses.  Same arithmetic per element; the parity tests compare the two. */
MMVAE_API int mmvae_net_set_join_grad(mmvae_net* net, int enable);
/* Which kernel route every block takes at batch size N, as text: one line per block (`encoder.layer1.0: fwd_c1_cs_stream=1 ...`,
 * `decoder.uplayer5.0: ...`) and a last line `net: ...` for the boundary layers, 0 / 1 per field (tail_fwd: GATHER, JOIN, STREAM or UP5); the
 * fields are DESIGN.md section 5's.  The routes are settled with the plan of N, before anything is enqueued: where the forward's and the
 * backward's routes do not fit each other this call and every network entry point return MMVAE_ERR_UNSUPPORTED and mmvae_last_error names the
 * rule.  Writes at most cap bytes (NUL-terminated) and returns the bytes needed, terminator included.  Host only: needs no device. */
MMVAE_API int mmvae_net_describe_routes(mmvae_net* net, int N, char* buf, int cap);

/* SyncBN: BatchNorm statistics over the global batch of a data-parallel job.  `fn` must SUM the `n` f32 values at
 * device pointer `buf` over all ranks in place, ordered on `stream` (the caller's stream or the net's side stream), and return 0;
 * it is called from inside the four network entry points, in the same order on every rank (two per BatchNorm and direction).
 * `world` = number of ranks; equal shards per rank are assumed (count = local count * world).  dgamma / dbeta stay per-rank
 * sums, like every other parameter gradient.  fn == NULL restores per-rank statistics. */
typedef int (*mmvae_allreduce_fn)(float* buf, int64_t n, void* stream, void* user);
MMVAE_API int mmvae_net_set_sync_bn(mmvae_net* net, mmvae_allreduce_fn fn, void* user, int world);

/* ------------------------------------------------------------------ data-parallel exchange (the reference has none,
 * main.py:433-437).  One RCCL communicator per process / GPU; RCCL is bound at run time (the copy already in the process,
 * else librccl.so / $MMVAE_RCCL_LIB).  Rank 0 creates the id, the host hands its 128 bytes to every rank (e.g. through the
 * torch.distributed store), every rank calls mmvae_comm_init (a collective).  mmvae_comm_allreduce: in-place f32 SUM over the
 * ranks, enqueued on `stream` (xGMI ring / tree chosen by RCCL); the gradient buckets and the SyncBN rows use it. */
typedef struct mmvae_comm mmvae_comm;
#define MMVAE_COMM_ID_BYTES 128
MMVAE_API int mmvae_comm_unique_id(void* id_host /* MMVAE_COMM_ID_BYTES, host */);
MMVAE_API int mmvae_comm_init(mmvae_comm** out, int world, int rank, const void* id_host);
MMVAE_API int mmvae_comm_allreduce(mmvae_comm* comm, float* buf, int64_t n, void* stream);
MMVAE_API int mmvae_comm_destroy(mmvae_comm* comm);
/* SyncBN through the communicator instead of a host callback: the row all-reduces are enqueued in-stream by the library.
 * comm == NULL restores per-rank statistics. */
MMVAE_API int mmvae_net_set_sync_bn_comm(mmvae_net* net, mmvae_comm* comm);
/* The rows are issued from TWO streams (the caller's and the net's side stream, which carries the shortcut branches), and a third
 * stream may carry the gradient buckets: RCCL orders the collectives of one communicator, so sharing one communicator would queue the
 * encoder's SyncBN rows behind the decoder's gradient bucket and relies on RCCL serialising concurrent streams.  This form gives the
 * rows of each stream a communicator of their own (both must differ from the one the gradient buckets use); on every rank each of
 * them sees its collectives in program order.  comm_side == NULL: side-stream rows use comm_main as well (the one-communicator form). */
MMVAE_API int mmvae_net_set_sync_bn_comm2(mmvae_net* net, mmvae_comm* comm_main, mmvae_comm* comm_side);

/* ------------------------------------------------------------------ latent + loss (model.py:148-150, :364-406)
 * Reparameterisation  enc = mu + eps * exp(0.5*logvar)  (VAE_Encoder.rsample, model.py:148-150). */
MMVAE_API int mmvae_rsample_fwd(const float* mu, const float* logvar, const float* eps, float* enc, int64_t n, void* stream);
MMVAE_API int mmvae_rsample_bwd(const float* d_enc, const float* logvar, const float* eps, float* d_mu, float* d_logvar, int64_t n,
                      void* stream);
/* The loss sums (kl_fwd, gauss_nll_fwd, ce_fwd, mmd_fwd) add into the f64 acc[0] with a reduction whose bits do not depend on
 * block arrival order, at any magnitude.  The *_ex forms take `partials`: device scratch of MMVAE_SUM_PARTIALS doubles whose first
 * word is zero before the first call (zero-fill it once).  Each block writes its f64 partial there and the last block to finish sums
 * them in block order and resets the first word, so the buffer is ready for the next call on the same stream (or a captured graph's
 * replay); calls that may run concurrently need buffers of their own.  The plain forms take no scratch and run the same sum in ONE
 * block: the same exactness and determinism, for small inputs (the train step uses the *_ex forms). */
#define MMVAE_SUM_PARTIALS 1025
/* acc[0] += -0.5*sum(logvar - exp(logvar) - mu^2 + 1)   (VAE.kl_divergence, model.py:364-365) */
MMVAE_API int mmvae_kl_fwd(const float* mu, const float* logvar, int64_t n, double* acc, void* stream);
MMVAE_API int mmvae_kl_fwd_ex(const float* mu, const float* logvar, int64_t n, double* acc, double* partials, void* stream);
/* d_mu = c*mu ; d_logvar = c*0.5*(exp(logvar)-1), c = coef * (gscale ? gscale[0] : 1).  In every *_bwd below `gscale` is an
 * optional DEVICE scalar (the upstream d(loss), so loss.backward() needs no host sync). */
MMVAE_API int mmvae_kl_bwd(const float* mu, const float* logvar, float coef, const float* gscale, float* d_mu, float* d_logvar, int64_t n,
                 void* stream);
/* acc[0] += -sum log N(target; recon, sigma)   (model.py:403); recon and target 16-byte aligned (else MMVAE_ERR_ARG) */
MMVAE_API int mmvae_gauss_nll_fwd(const float* recon, const float* target, int64_t n, float sigma, double* acc, void* stream);
MMVAE_API int mmvae_gauss_nll_fwd_ex(const float* recon, const float* target, int64_t n, float sigma, double* acc, double* partials,
                                     void* stream);
MMVAE_API int mmvae_gauss_nll_bwd(const float* recon, const float* target, int64_t n, float sigma, float coef, const float* gscale,
                        float* d_recon, void* stream);
/* acc[0] += sum w[t]*CE(recon[:, :, p], t)   (F.cross_entropy(reduction='none', weight).sum(), model.py:400-401);
 * recon [N,Q,HW] f32, target [N,HW] int64, weight [Q] f32 or NULL */
MMVAE_API int mmvae_ce_fwd(const float* recon, const int64_t* target, const float* weight, int N, int Q, int HW, double* acc, void* stream);
MMVAE_API int mmvae_ce_fwd_ex(const float* recon, const int64_t* target, const float* weight, int N, int Q, int HW, double* acc,
                              double* partials, void* stream);
MMVAE_API int mmvae_ce_bwd(const float* recon, const int64_t* target, const float* weight, int N, int Q, int HW, float coef,
                 const float* gscale, float* d_recon, void* stream);
/* acc[0] += sum k(x,x) + sum k(y,y) - 2 sum k(x,y),  k(a,b) = exp(-|a-b|^2 / d^2)   (compute_mmd, model.py:367-383);
 * x = true_samples, y = encoding, both [n,d] f32.  Never materialises (n,n,d).  scratch: 2n floats (row norms) selects the
 * exact-f32 MFMA path |x|^2+|y|^2-2x.y (x and y 16-byte aligned, else MMVAE_ERR_ARG); NULL the direct (x-y)^2 VALU path. */
MMVAE_API int mmvae_mmd_fwd(const float* x, const float* y, int n, int d, float* scratch, double* acc, void* stream);
MMVAE_API int mmvae_mmd_fwd_ex(const float* x, const float* y, int n, int d, float* scratch, double* acc, double* partials, void* stream);
/* d_y += coef * d(mmd)/dy; d <= 512 (else MMVAE_ERR_UNSUPPORTED) */
MMVAE_API int mmvae_mmd_bwd(const float* x, const float* y, int n, int d, float coef, const float* gscale, float* d_y, void* stream);
/* k[i][j] = exp(-mean_d((x_i - y_j)^2) / d), out (n, m) f32   (VAE.compute_kernel, model.py:367-376) */
MMVAE_API int mmvae_rbf_kernel(const float* x, const float* y, int n, int m, int d, float* out, void* stream);
/* acc = {px, kl, mmd} (f64) -> out[4] = {(nll*px + kl_coef*kl + mmd_coef*mmd)/n, nll*px/n, kl/n, mmd/n}  (model.py:405-406) */
MMVAE_API int mmvae_loss_finish(const double* acc, float* out, float nll, float kl_coef, float mmd_coef, float n, void* stream);

/* ------------------------------------------------------------------ held-out evaluation: per-image terms
 * Every output is f64 [N], one value per image, WRITTEN (not accumulated) in a fixed order by one block per image: two calls on
 * the same inputs return the same bits.  No alignment is required of any pointer beyond its element type's.  A NULL pointer
 * (`weight` excepted), a non-positive N, per, Q, HW, d or K, or sigma <= 0 returns MMVAE_ERR_ARG with nothing enqueued.
 * out[n] = -sum_{i < per} log N(target[n][i]; recon[n][i], sigma)   (the per-image share of mmvae_gauss_nll_fwd) */
MMVAE_API int mmvae_gauss_nll_per_image(const float* recon, const float* target, int N, int64_t per, float sigma, double* out, void* stream);
/* out[n] = sum_pix weight[t] * (logsumexp_q recon[n][:][pix] - recon[n][t][pix]), t = target[n][pix]; recon [N,Q,HW] f32, target [N,HW]
 * int64 in [0, Q), weight [Q] f32 or NULL   (the per-image share of mmvae_ce_fwd) */
MMVAE_API int mmvae_ce_per_image(const float* recon, const int64_t* target, const float* weight, int N, int Q, int HW, double* out, void* stream);
/* out[n] = -0.5 * sum_{i < d} (logvar - exp(logvar) - mu^2 + 1); mu, logvar [N,d] f32 */
MMVAE_API int mmvae_kl_per_image(const float* mu, const float* logvar, int N, int d, double* out, void* stream);
/* out[n] = log p(z) - log q(z|x) = -0.5 * sum_{i < d} (z^2 - eps^2 - logvar), z = mu + exp(logvar/2) * eps: the f32 code
 * mmvae_rsample_fwd produces from the same inputs, p the standard normal prior */
MMVAE_API int mmvae_latent_logratio(const float* mu, const float* logvar, const float* eps, int N, int d, double* out, void* stream);
/* Importance-weighted bound from K samples: nll, logratio f64 [K][N] (row k: the two calls above for sample k);
 * out[n] = logsumexp_k(logratio[k][n] - nll[k][n]) - log K, the maximum subtracted before any exponential.  K = 1 returns
 * logratio - nll to the last bit. */
MMVAE_API int mmvae_iw_bound(const double* nll, const double* logratio, int K, int N, double* out, void* stream);

/* ------------------------------------------------------------------ train-step plumbing
 * (label - mean)/std, main.py:383-387.  labels int64 [n]; image f32 [n]. */
MMVAE_API int mmvae_normalise_labels(const int64_t* labels, int64_t n, float mean, float stdv, float* image, void* stream);
/* Input pipeline on device: uint8 pixel -> x/255 -> nearest of q k-means centres (kmeans.predict, main.py:25,
 * utils.py:279-309; lowest index wins ties) -> labels int64 (may be NULL) and image = (label-mean)/std f32 (may be NULL). */
MMVAE_API int mmvae_quantise_normalise(const uint8_t* frames, int64_t n, const float* centres, int q, float mean, float stdv,
                             int64_t* labels, float* image, void* stream);
/* Fitting that quantiser (utils.save_kmeans_file, utils.py:279-309).  Everything the reference derives by sampling is an exact function
 * of the byte histogram of the data, taken in one pass on the device:
 * counts[b] += occurrences of byte b.  clip_index == NULL: the bytes [0, n_clips * clip_bytes) of frames; otherwise the n_clips clips
 * frames + clip_index[i] * clip_bytes (device int64; repeats are counted again; the CALLER keeps every index inside the buffer).
 * counts: 256 device uint64, ADDED to (the caller zeroes them; several buffers may share one histogram).  frames and clip_bytes may
 * have any alignment.  n_clips == 0 is a no-op.  Integer atomics only: the same bits every run. */
MMVAE_API int mmvae_u8_histogram(const uint8_t* frames, int64_t clip_bytes, const int64_t* clip_index, int64_t n_clips, uint64_t* counts,
                       void* stream);
/* HOST function, every pointer host memory: exact weighted k-means of the 256 byte values b/255 (weights counts[b]) into q clusters by
 * dynamic programming over contiguous partitions of the non-empty bins (ties: the smallest cut index).  centres[q]: the weighted means,
 * ASCENDING, on the ToTensor scale -- label k is the k-th darkest cluster, where scikit-learn's label order is arbitrary (data_mean /
 * data_std below depend on the order).  inertia (may be NULL): sum_b counts[b] (b/255 - centre(b))^2.  MMVAE_ERR_ARG: q < 1, q > 256,
 * all counts zero, q > the number of distinct values present (the message names it); MMVAE_ERR_UNSUPPORTED: more than 2^64 / 255^2
 * pixels. */
MMVAE_API int mmvae_kmeans1d_fit(const uint64_t* counts, int q, double* centres, double* inertia);
/* HOST function: lut[b] = the label mmvae_quantise_normalise gives byte b with these f32 centres (the kernel's own f32 arithmetic and
 * tie rule), and from counts and lut in f64: ratios[q] (class frequencies, utils.py:296-297), the mean and the POPULATION std of the
 * labels (utils.py:298-299: main.py's data_mean / data_std, unrounded).  ratios, label_mean, label_std may be NULL. */
MMVAE_API int mmvae_quantiser_stats(const uint64_t* counts, const float* centres, int q, uint8_t* lut, double* ratios, double* label_mean,
                          double* label_std);
/* The resize branch of the input transform (choose_transformer, main.py:33-38: ToPILImage -> Resize(S) -> ToTensor -> kmeans.predict).
 * transforms.Resize is Pillow's 8-bit antialiased bilinear resample; a byte that is off by one next to a k-means boundary is another
 * label, so the two calls below reproduce Pillow's bytes exactly.
 * HOST function, every pointer host memory: the taps of ONE axis, in_size -> out_size, both in [1, 128] (else MMVAE_ERR_ARG), computed as
 * Pillow's precompute_coeffs / normalize_coeffs_8bpc do (f64, triangle filter of support max(in / out, 1), weights divided by their
 * sum, rounded to 22-bit fixed point).  *ksize = taps per output.  bounds [out_size][2] = {first input index, tap count <= ksize};
 * coeffs [out_size][ksize], zero behind the tap count.  bounds == coeffs == NULL: only *ksize is written (size the buffers with it).
 * A pass is out = clamp((2^21 + sum_x pixel[first + x] * coeffs[x]) >> 22, 0, 255); int32 suffices. */
MMVAE_API int mmvae_resample_coeffs(int in_size, int out_size, int* ksize, int32_t* bounds, int32_t* coeffs);
/* Resize + mmvae_quantise_normalise in one launch.  n_frames uint8 planes of in_h x in_w (rows contiguous, planes frame_stride_bytes
 * apart, any alignment: 16-byte aligned frames and stride take the vector loads) are resized to out_h x out_w as Pillow mode-L images --
 * the horizontal pass along in_w first, uint8 rounding behind each pass -- then quantised by mmvae_quantise_normalise's own f32 rule:
 * for the same resized bytes the outputs equal that call's bit for bit.  Plane p is plane p % frames_per_clip of clip
 * clip_index[p / frames_per_clip] (device int64, a gather of whole clips from a resident dataset; the CALLER keeps every index inside
 * the buffer), or of clip p / frames_per_clip when clip_index is NULL (frames_per_clip = 1: plane p).  h_* are the DEVICE copies of
 * mmvae_resample_coeffs(in_w, out_w), v_* of (in_h, out_h); h_ksize / v_ksize must be the values that call returns.  centres: q f32,
 * needed for labels or image.  Outputs, dense [n_frames][out_h][out_w], each may be NULL but not all three (MMVAE_ERR_ARG): labels
 * int64, image = ((float)label - mean) / stdv f32, resized uint8 (the bytes themselves).  n_frames == 0 is a no-op.  No atomics: the
 * same bits every run. */
MMVAE_API int mmvae_resize_quantise_normalise(const uint8_t* frames, int64_t frame_stride_bytes, const int64_t* clip_index,
                                              int frames_per_clip, int64_t n_frames, int in_h, int in_w, int out_h, int out_w,
                                              const int32_t* h_bounds, const int32_t* h_coeffs, int h_ksize, const int32_t* v_bounds,
                                              const int32_t* v_coeffs, int v_ksize, const float* centres, int q, float mean, float stdv,
                                              int64_t* labels, float* image, uint8_t* resized, void* stream);
/* ------------------------------------------------------------------ data generator
 * Moving MNIST is not a fixed corpus but a recipe (Srivastava et al. 2015): K glyphs bounce inside an S x S canvas for T frames and
 * overlaps are composited with max.  The reference reads movingmnist{train,test}.npz and neither ships them nor says how they were made;
 * this call makes the clips, on the device, at the rate the train step consumes them.  THE RULE BELOW IS PART OF THE INTERFACE: clip c
 * is a pure function of (seed, c, bank, parameters), the same bits on every run, for every n_clips, first_clip split and launch
 * geometry, so a file made from a seed can be made again.  It is stated in integers throughout.
 *
 * Parameters: S canvas side, a multiple of 16 in 16..64; G glyph side, 1..MMVAE_CLIPGEN_MAX_G; R = S - G >= 1; T frames,
 * 1..MMVAE_CLIPGEN_MAX_T; K digits per clip, 1..MMVAE_CLIPGEN_MAX_K; D glyphs in the bank, 1..MMVAE_CLIPGEN_MAX_D (outside these:
 * MMVAE_ERR_UNSUPPORTED, the message names the parameter).  bank: uint8 [D][G][G], any alignment.
 *
 * Random numbers (uint64, wrap-around):  mix64(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 * z ^= z >> 31.  For clip c >= 0 and digit k: n = 8c + k, GOLD = 0x9E3779B97F4A7C15, r1 = mix64(seed + GOLD * (2n + 1)),
 * r2 = mix64(seed + GOLD * (2n + 2)).  Draws: glyph g = ((r1 >> 32) * D) >> 32; x = r2 & 0xFFFF; y = (r2 >> 16) & 0xFFFF; direction
 * a = (r2 >> 32) & 0xFFF.
 *
 * Velocity: (vx, vy) = (vel[a][0], vel[a][1]), vel a DEVICE int32 table [MMVAE_CLIPGEN_DIRECTIONS][2] the caller computes once per speed
 * in f64: vx[a] = rint(speed * 65536 * cos(2 pi a / 4096)), vy[a] the same with sin; speed in (0, 1] is the fraction of the free range
 * travelled per frame (0.1 in the canonical data).  The device only reads the table (|entry| <= 65536 is the CALLER's promise).
 *
 * Trajectory: int32 coordinates, ONE = 65536 the whole free range.  For t = 0 .. T-1, update first, record afterwards:
 *   x += vx; y += vy;  if (x <= 0) { x = 0; vx = -vx; }  if (x >= ONE) { x = ONE; vx = -vx; }  the same for y;
 *   the glyph's top-left pixel in frame t is px = (x * R) >> 16, py = (y * R) >> 16, both in [0, R].
 *
 * Frame: out[c][t][row][col] = max over k of bank[g_k][row - py_k][col - px_k] where that index lies inside the glyph, else 0.
 *
 * Clips first_clip .. first_clip + n_clips - 1 (first_clip >= 0) are written; outputs are dense [n_clips][T][S][S], 16-byte aligned,
 * each may be NULL but not all three (MMVAE_ERR_ARG): bytes uint8 (what MovingMNISTClips holds: (N, C, H, W)), and labels int64 /
 * image f32 = exactly what mmvae_quantise_normalise(centres, q, mean, stdv) gives for those bytes, bit for bit (centres: q f32, needed
 * for labels or image only).  n_clips == 0 is a no-op.  One launch on `stream`; no atomics, no scratch, no host read. */
#define MMVAE_CLIPGEN_MAX_G 32
#define MMVAE_CLIPGEN_MAX_T 32
#define MMVAE_CLIPGEN_MAX_K 4
#define MMVAE_CLIPGEN_MAX_D (1 << 24)
#define MMVAE_CLIPGEN_DIRECTIONS 4096
MMVAE_API int mmvae_generate_clips(const uint8_t* bank, int64_t D, int G, const int32_t* vel, uint64_t seed, int64_t first_clip,
                                   int64_t n_clips, int T, int S, int K, const float* centres, int q, float mean, float stdv,
                                   int64_t* labels, float* image, uint8_t* bytes, void* stream);
/* ------------------------------------------------------------------ picture panels (the plot branch, main.py:205-359, utils.py:77-83)
 * Pick rule, shared by the two calls below: the Q f32 logits of one pixel -> a label in [0, Q).  1 <= Q <= 16 (else
 * MMVAE_ERR_UNSUPPORTED).  MMVAE_PICK_ARGMAX: the lowest index among equal maxima (strict > scan from index 0; a NaN never wins, an
 * all-NaN pixel gives 0).  MMVAE_PICK_SAMPLE: f32 softmax (maximum subtracted, expf, sum in channel order), then
 * label = #{k in [0, Q-2] : cdf_k <= u}, cdf accumulated in channel order -- the draw rule of mmvae_pixelcnn_sample. */
#define MMVAE_PICK_ARGMAX 0
#define MMVAE_PICK_SAMPLE 1
/* logits f32 planar [N][Q][HW] (what the forward passes return); uniforms f32 [N][HW] in [0, 1), read in sample mode only (may be NULL
 * otherwise); labels int64 [N][HW]. */
MMVAE_API int mmvae_logits_to_labels(const float* logits, int N, int Q, int HW, int mode, const float* uniforms, int64_t* labels,
                                     void* stream);
/* One column of a contact sheet: n planes of S x S.  src by kind:
 *   LABELS_U8 / LABELS_I64  [n][S*S]: byte = lut[label]; a label outside [0, Q) gives 0;
 *   LOGITS_ARGMAX / _SAMPLE [n][Q][S*S] f32: the pick rule above (uniforms [n][S*S] for _SAMPLE), then lut;
 *   IMAGE_F32               [n][S*S] f32: x = (v - lo) / (hi - lo) * 255 in f32, byte = clamp(floor(x + 0.5), 0, 255), NaN gives 0; needs
 *                           hi > lo; Q, lut and uniforms are ignored.
 * lut: Q device bytes (the grey of each class). */
#define MMVAE_PANEL_LABELS_U8 0
#define MMVAE_PANEL_LABELS_I64 1
#define MMVAE_PANEL_LOGITS_ARGMAX 2
#define MMVAE_PANEL_LOGITS_SAMPLE 3
#define MMVAE_PANEL_IMAGE_F32 4
#define MMVAE_PANEL_MAX_COLS 8
typedef struct mmvae_panel_col {
  int32_t kind;
  const void* src;
  int32_t Q;
  const float* uniforms;
  const uint8_t* lut;
  float lo, hi;
} mmvae_panel_col;
/* The whole sheet in one launch: out uint8 [n * S][ncols * S], row-major; column c fills bytes [:, c*S : (c+1)*S] with its n planes
 * stacked vertically (the reference's x[:6].view(-1, S) strip).  cols: HOST array of ncols descriptors, copied into the launch (it may
 * be freed when the call returns); the pointers inside are device pointers.  1 <= ncols <= MMVAE_PANEL_MAX_COLS, n >= 1,
 * 1 <= S <= 64.  Every byte of out is written exactly once, none outside it; no atomics: the same bytes every run. */
MMVAE_API int mmvae_panel_sheet(const mmvae_panel_col* cols, int ncols, int n, int S, uint8_t* out, void* stream);

/* ------------------------------------------------------------------ per-frame quality: squared error and SSIM of two columns
 * n pairs of S x S planes, 11 <= S <= 64 (else MMVAE_ERR_UNSUPPORTED), one launch.  a and b: one HOST descriptor each, copied into the
 * launch; each side is reduced to bytes by the column rule above (the bytes mmvae_panel_sheet would write for it), or is bytes already:
 *   MMVAE_FRAME_BYTES_U8 [n][S*S] uint8, taken as is; the other fields of the descriptor are ignored.  This kind is accepted here only:
 *   mmvae_panel_sheet refuses it.
 * Per plane pair p, with a and b the two byte planes as exact values:
 *   out[p]     = sse  = sum over the S*S pixels of (a - b)^2, an integer <= 4096 * 65025, exact in f64;
 *   out[n + p] = ssim = the mean over the (S - 10)^2 positions whose 11 x 11 window lies inside the plane of
 *                  ((2 mu_a mu_b + C1) (2 s_ab + C2)) / ((mu_a^2 + mu_b^2 + C1) (s_a^2 + s_b^2 + C2)),
 *     mu_a = E[a], mu_b = E[b], s_a^2 = E[a^2] - mu_a^2, s_b^2 = E[b^2] - mu_b^2, s_ab = E[a b] - mu_a mu_b, every E[.] the sum under
 *     the window w = g g^T, g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)) / sum_k (k = 0..10), C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2.
 *   This is Wang et al. 2004 on 8-bit data; it is what skimage.metrics.structural_similarity(gaussian_weights=True,
 *   use_sample_covariance=False, data_range=255) returns, whose border crop leaves the same positions.
 * All arithmetic is f64 (window sums, map, mean; g is computed once on the host in double); mse = sse / S^2 and
 * psnr = 10 log10(65025 / mse) are the caller's.  out: f64 [2][n]; nothing outside it is written.  No atomics, no allocation, no host
 * read: capturable, and the same bits every run.
 * MMVAE_ERR_ARG, nothing enqueued: NULL a, b, out or source, n < 1, an unknown kind, a class kind without lut (or _SAMPLE without
 * uniforms) or with Q outside 1..16, IMAGE_F32 without hi > lo. */
#define MMVAE_FRAME_BYTES_U8 5
MMVAE_API int mmvae_frame_quality(const mmvae_panel_col* a, const mmvae_panel_col* b, int n, int S, double* out, void* stream);

/* ------------------------------------------------------------------ latent diagnostics (scatter_plot, main.py:166-183)
 * Density panel of n 2-D points, the picture behind the reference's scatter plot of q(z|x) against p(z): point p is
 * (pts[p*stride + col_x], pts[p*stride + col_y]) (an (N, z, 1, 1) encoding in place: stride = z; the reference plots dimensions 0, 1).
 * xform: 4 DEVICE floats {xlim, ylim, sx, sy} (the caller computes the limits with tensor operations, no host read; sx = 8*side/xlim,
 * sy = 8*side/ylim map [-lim, lim] onto 16 sub-positions per pixel; the kernel does not recompute them).  In f32, in exactly this order
 * (an add, then a multiply: nothing contracts to an fma):
 *   qx = (int)floorf((x + xlim) * sx),   qy = (int)floorf((ylim - y) * sy)          (y points up)
 * Pixel (row i, column j) is covered by the point iff (16 j + 8 - qx)^2 + (16 i + 8 - qy)^2 <= radius16^2, in integers.  With k(i, j) the
 * number of covering points, out[i * out_row_stride + j] = tone[min(k, 255)] for 0 <= i, j < side (tone: 256 device bytes): every byte of
 * the panel is written, none outside it (the row stride lets two panels share a sheet).  A point with a non-finite coordinate, or whose
 * disc misses the panel, is skipped; a huge finite value cannot overflow.  n = 0 gives tone[0] everywhere.  One launch, integer counts
 * in LDS: no global atomics, no zero-filled buffer, the same bytes every run and for every order of the points.
 * side: a multiple of 16 in [16, 512], radius16 in [12, 128] (sixteenths of a pixel; at 12 every point inside the panel covers its own
 * pixel) -- else MMVAE_ERR_UNSUPPORTED; n >= 0, stride >= 1, 0 <= col_x, col_y < stride, out_row_stride >= side, no NULL pointer (pts
 * may be NULL when n = 0) -- else MMVAE_ERR_ARG.  Nothing is enqueued on an error.
 * This is a density image under the rule above, not a pixel copy of a matplotlib figure (no antialiased marker edges, axes or labels). */
MMVAE_API int mmvae_scatter_panel(const float* pts, int64_t n, int stride, int col_x, int col_y, const float* xform, int side, int radius16,
                                  const uint8_t* tone, uint8_t* out, int64_t out_row_stride, void* stream);
/* Per-dimension sums over the N images of a batch, acc f64 [6][d]; mu, logvar, enc f32 [N][d]; every term is formed in double from the
 * f32 inputs.  Rows: 0 sum mu, 1 sum mu^2, 2 sum 0.5 (exp(logvar) + mu^2 - logvar - 1) (the KL of each dimension), 3 sum exp(logvar),
 * 4 sum enc, 5 sum enc^2.  logvar NULL: rows 2, 3 are zero; enc NULL: rows 4, 5 are zero.  accumulate = 0 writes the rows, 1 adds to
 * what is there (carry one accumulator over a data loader).  Fixed order, no atomics: the bits depend on the inputs only.
 * 1 <= d <= 512 (else MMVAE_ERR_UNSUPPORTED), N >= 1, accumulate in {0, 1}, mu and acc not NULL (else MMVAE_ERR_ARG). */
MMVAE_API int mmvae_latent_stats(const float* mu, const float* logvar, const float* enc, int N, int d, int accumulate, double* acc,
                                 void* stream);

/* ------------------------------------------------------------------ aggregate-posterior densities (ELBO surgery, Hoffman & Johnson 2016)
 * N samples z [N][d] against a bank of M diagonal Gaussian posteriors mu, logvar [M][d] (dense f32 device arrays):
 *   t_ijd = -0.5 * ((z_id - mu_jd)^2 * exp(-logvar_jd) + logvar_jd + log(2 pi)),      s_ij = sum_d t_ijd,
 *   log_qz[i]         = logsumexp_j s_ij  - log M        f64 [N]     (log of the aggregate posterior q(z) = mean_j q(z | x_j) at z_i)
 *   log_qz_dims[i][d] = logsumexp_j t_ijd - log M        f64 [N][d]  (log of its d-th marginal), skipped when log_qz_dims is NULL.
 * Every maximum is subtracted before any exponential is taken (an online log-sum-exp over groups of 8 bank rows).
 * Precision: the terms are formed in f32 from the f32 inputs (exp(-logvar) and the additive constant of a bank entry are formed in f64
 * and rounded once to f32; the arithmetic runs in the base-2 domain).  Sums of exponentials are f32 over the 8 rows of a group only and
 * f64 from there on; the joint's sum over d is f32 inside a tile of at most 32 dimensions and f64 across tiles.  The outputs are f64.
 * Outputs and determinism: every element of log_qz (and of log_qz_dims) is written, nothing is accumulated into what was there.  The bank
 * is cut into chunks of rows by a rule that depends on (N, M, d) alone; the (max, sum) pairs of the chunks go through `scratch` and are
 * combined in chunk order in f64; with a single chunk the sweep writes the output itself by the same formula.  No atomics: the same bits
 * every run.  Every scratch word that is read was written earlier by the same call, so the scratch may hold anything on entry.  No
 * allocation, no host read, no synchronisation: a handful of launches on `stream`, capturable.  log_qz has the same bits whether or not
 * log_qz_dims is asked for.
 * scratch: 16-byte aligned device memory of at least mmvae_posterior_mixture_scratch_bytes(N, M, d) bytes (a function of the shape
 * alone, 0 for a shape the call refuses): the re-laid bank (12 bytes per bank entry), the padded samples and the chunk pairs.
 * Ranges: 1 <= d <= 512, 1 <= N, M <= 2^20; above them MMVAE_ERR_UNSUPPORTED.  A non-positive N, M or d, a NULL pointer (log_qz_dims may
 * be NULL), a misaligned or too-small scratch: MMVAE_ERR_ARG.  Nothing is enqueued on an error.
 * Domain: |z|, |mu| <= 1e4 and |logvar| <= 30.  Inside it every term is finite in f32 (at most about 4e21 in magnitude), the running
 * maximum is finite and no NaN appears.  Outside it (and for non-finite inputs) the output values are unspecified; nothing is written
 * out of bounds. */
MMVAE_API size_t mmvae_posterior_mixture_scratch_bytes(int N, int M, int d);
MMVAE_API int mmvae_posterior_mixture(const float* z, int N, const float* mu, const float* logvar, int M, int d, double* log_qz,
                                      double* log_qz_dims, void* scratch, size_t scratch_bytes, void* stream);
/* The gradient of both outputs with respect to z, mu and logvar (training against the split: the beta-TCVAE penalty of Chen et al. 2018).
 * z, mu, logvar as above; log_qz f64 [N] and log_qz_dims f64 [N][d] are the outputs mmvae_posterior_mixture wrote for these very inputs;
 * g_joint f64 [N] and g_dims f64 [N][d] are the upstream gradients of log_qz and log_qz_dims.  Either g may be NULL, meaning zero, but
 * not both; log_qz_dims may be NULL if and only if g_dims is NULL.  With
 *   r_ij   = exp(s_ij  - (log_qz[i]         + log M))       (sum_j r_ij = 1)
 *   rd_ijd = exp(t_ijd - (log_qz_dims[i][d] + log M))
 *   a_ijd  = g_joint[i] * r_ij + g_dims[i][d] * rd_ijd
 *   u_ijd  = (z_id - mu_jd) * exp(-logvar_jd)
 * the outputs, dense f32 device arrays, are
 *   d_z[i][d]      = - sum_j a_ijd * u_ijd                              [N][d]
 *   d_mu[j][d]     =   sum_i a_ijd * u_ijd                              [M][d]
 *   d_logvar[j][d] =   sum_i a_ijd * 0.5 * ((z_id - mu_jd) * u_ijd - 1) [M][d]
 * Every element of the three is written, nothing is accumulated into what was there, and nothing outside them and the scratch is written.
 * Determinism: d_z is a sum over the bank and d_mu / d_logvar are sums over the samples; each is taken by a sweep of its own that keeps
 * one output row per lane (the other side is staged through LDS), cut into chunks by a rule that depends on (N, M, d) alone; the chunks'
 * partial sums go through `scratch` and are combined in chunk order.  Fixed summation order, no atomics: the same bits every run.
 * Precision: the terms are formed in f32 (the bank entries as in the forward; g_joint, g_dims and log_qz_dims + log M are rounded once to
 * f32, log_qz + log M stays f64 and is subtracted from the f64 joint exponent).  No f32 sum is carried over more than the 8 terms of a
 * group (16 inside a tile of the joint exponent); every longer sum is f64 and is rounded once to f32 at the store.
 * Capturable: no allocation, no host read, no synchronisation; five launches on `stream`.
 * scratch: 16-byte aligned device memory of at least mmvae_posterior_mixture_bwd_scratch_bytes(N, M, d) bytes (a function of the shape
 * alone, 0 for a shape the call refuses).  Every scratch word that is read was written earlier by the same call.
 * Ranges: 1 <= d <= 512 and 1 <= N, M <= 16384 (training batches; evaluation-size banks are not the use); above them
 * MMVAE_ERR_UNSUPPORTED.  A non-positive N, M or d, a NULL required pointer, both g_joint and g_dims NULL, g_dims without log_qz_dims, a
 * misaligned or too-small scratch: MMVAE_ERR_ARG.  Nothing is enqueued on an error, and mmvae_last_error() names the value.
 * Domain: the forward's, |z|, |mu| <= 1e4 and |logvar| <= 30, with log_qz / log_qz_dims the forward's outputs and finite upstream
 * gradients.  Inside it every output is finite: the largest u is about 2e17 and the largest (z - mu) * u about 4e21, both finite in
 * f32, and a weight that underflows to 0 multiplies a finite number.  Outside it the output values are unspecified; nothing is written
 * out of bounds. */
MMVAE_API size_t mmvae_posterior_mixture_bwd_scratch_bytes(int N, int M, int d);
MMVAE_API int mmvae_posterior_mixture_bwd(const float* z, int N, const float* mu, const float* logvar, int M, int d, const double* log_qz,
                                          const double* log_qz_dims, const double* g_joint, const double* g_dims, float* d_z, float* d_mu,
                                          float* d_logvar, void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------ nearest training frames of a sample (memorised or drawn?)
 * Exact k nearest neighbours of M query planes among F resident frames.  queries [M][D], frames [F][D]: dense device uint8, 16-byte
 * aligned.  d(m, f) = sum_{i<D} (queries[m][i] - t(frames[f][i]))^2 with t the identity when lut is NULL and lut[.] (256 device bytes)
 * otherwise: the lut is applied to `frames` only, the caller hands `queries` already in the compared space.  Exact integer arithmetic
 * (D * 255^2 <= 16384 * 65025 = 1 065 369 600 fits int32); no floating point is used anywhere.  For every query the frames are ordered by
 * the pair (d, f) ascending -- equal distances fall to the lower frame index -- and the first k go to out_dist[m][0..k) (int32) and
 * out_index[m][0..k) (int64).  Every output element is written exactly once, none outside the [M][k] arrays, nothing outside
 * scratch_bytes of `scratch` (16-byte aligned device memory of at least mmvae_nearest_frames_scratch_bytes(M, F, D, k) bytes, a function
 * of the shape alone; 0 for a shape the call refuses).  The same bits come out every run, whatever the grid.
 * Supported: 1 <= M <= 64, 1 <= k <= 8, k <= F <= 2^31 - 1, D a multiple of 16 in [16, 16384].  A non-positive M, F, D or k, k > F, a
 * NULL or misaligned pointer (lut may be NULL): MMVAE_ERR_ARG; a too-small scratch: MMVAE_ERR_WORKSPACE; M > 64, k > 8, any other D,
 * F > 2^31 - 1: MMVAE_ERR_UNSUPPORTED.  On an error nothing is enqueued and mmvae_last_error() names the offending value. */
MMVAE_API size_t mmvae_nearest_frames_scratch_bytes(int M, int64_t F, int D, int k);
MMVAE_API int mmvae_nearest_frames(const uint8_t* queries, int M, const uint8_t* frames, int64_t F, int D, const uint8_t* lut, int k,
                                   int32_t* out_dist, int64_t* out_index, void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------ set-to-set k-NN and ball counts (sample-quality scores)
 * Every row of a [Na][D] against every row of b [Nb][D]: dense device uint8, 16-byte aligned.  d(i, j) = sum_{t<D} (a[i][t] - b[j][t])^2
 * in exact integer arithmetic (D * 255^2 <= 1 065 369 600 fits int32); no floating point is used anywhere.  Up to two results per row
 * of a:
 *   the k nearest (k in 1..8): the columns are ordered by the pair (d, j) ascending -- equal distances fall to the lower index -- and the
 *     first k go to out_dist[i][0..k) (int32) and out_index[i][0..k) (int64).  k = 0 with out_dist = out_index = NULL: no selection.
 *   the ball count: with col_radius (int32 [Nb], every entry >= 0) and out_count (int32 [Na]),
 *     out_count[i] = #{ j : d(i, j) <= col_radius[j] }, the comparison inclusive and exact.  Both pointers or neither.
 * A call asks for at least one of the two.  exclude_diagonal != 0 removes the pairs (i, i) from both results (leave-one-out when a and b
 * are the same set); it requires k <= Nb - 1.
 * Every output element is written exactly once, none outside the [Na][k] / [Na] arrays, nothing outside scratch_bytes of `scratch`
 * (16-byte aligned device memory of at least mmvae_knn_cross_scratch_bytes(Na, Nb, D, k, want_count) bytes, a function of the shape
 * alone; 0 for a shape the call refuses; want_count != 0 when out_count is given).  Determinism: a block owns 128 rows of a and a
 * contiguous range of columns; its partial k-best lists are keyed (d << 32) | j and merged by key, its partial counts are summed as
 * integers in a fixed order.  No floating-point atomics: the same bits every run, whatever the grid and however the columns are split.
 * Capturable: no allocation, no host read, no synchronisation; three launches on `stream`.
 * Supported: 1 <= Na, Nb <= 2^20, 0 <= k <= 8, D a multiple of 16 in [16, 16384].  A non-positive Na, Nb or D, a negative k, k above the
 * available columns (Nb, or Nb - 1 with exclude_diagonal), a NULL or misaligned a, b or scratch, col_radius without out_count or the
 * reverse, out_dist / out_index not both given with k > 0 or not both NULL with k = 0, nothing asked for: MMVAE_ERR_ARG; a too-small
 * scratch: MMVAE_ERR_WORKSPACE; Na or Nb > 2^20, k > 8, any other D: MMVAE_ERR_UNSUPPORTED.  On an error nothing is enqueued and
 * mmvae_last_error() names the offending value.  A negative col_radius entry is not an error of the call: that column is in no ball. */
MMVAE_API size_t mmvae_knn_cross_scratch_bytes(int64_t Na, int64_t Nb, int D, int k, int want_count);
MMVAE_API int mmvae_knn_cross(const uint8_t* a, int64_t Na, const uint8_t* b, int64_t Nb, int D, int k, int exclude_diagonal,
                              int32_t* out_dist, int64_t* out_index, const int32_t* col_radius, int32_t* out_count, void* scratch,
                              size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------ per-tensor histograms of a flat buffer (wandb.hook_torch, main.py:456)
 * 64-bin histograms and exact statistics of T segments of one flat f32 device buffer -- every parameter's gradient, weight or Adam
 * moment in one call.  segments: T pairs (offset, numel) of int64, in elements of `flat`; any alignment, gaps and numel = 0 allowed.
 * chunks: n_chunks triples (segment, start, length) of int64 -- the unit of work, one block each; the chunks of a segment must tile
 * [0, numel) exactly once (mmvae_tensor_hist_chunks builds such a list; an element no chunk covers is not counted, one covered twice is
 * counted twice).  Both tables are passed twice: the HOST copy is checked before anything is enqueued, the DEVICE copy is what the
 * kernels read; they must hold the same values.
 * Per segment t, every operation a correctly rounded f32 operation:
 *   lo, hi = min / max over the FINITE elements.  No finite element (or numel = 0): lo[t] = hi[t] = 0, all counts 0.
 *   lo == hi: the range becomes lo - 1 .. hi + 1 (torch.histc), and that is what lo[t], hi[t] report.
 *   a finite x goes to bin min((int)(((x - lo) * 64.0f) / (hi - lo)), 63)   (ATen's device histc: multiply first, an IEEE division);
 *   NaN and +-inf are counted in n_nonfinite and in no bin.  The bin index is clamped to 0..63 whatever the data; the counts of a range
 *   whose width overflows f32 (or of a constant so large that lo - 1 == lo) are unspecified, nothing is written out of bounds.
 * counts int32 [T][64], lo / hi f32 [T], stats f64 [T][MMVAE_TENSOR_HIST_STATS]: n_finite, n_nonfinite, n_zero (finite and == 0, either
 * sign), sum and sum of squares of the finite values (terms formed in f64), mean = sum / n_finite, rms = sqrt(sumsq / n_finite) (0 when
 * n_finite = 0), 0.  Every output element is written by every call.  Three launches on `stream` (per-chunk range and sums, a
 * per-segment finalize in a fixed order, per-chunk bins merged with integer atomics): no host read, no allocation, no floating-point
 * atomics -- capturable, and the same input gives the same bits every run.
 * scratch: at least mmvae_tensor_hist_scratch_bytes(T, n_chunks) bytes of 8-byte aligned device memory.
 * Errors, nothing enqueued: a NULL pointer (chunks / chunks_dev may be NULL when n_chunks = 0), T <= 0, n_chunks < 0, a negative offset
 * or numel, a segment that leaves [0, flat_numel), a chunk of an unknown segment or one that leaves its segment: MMVAE_ERR_ARG; a
 * too-small scratch: MMVAE_ERR_WORKSPACE. */
#define MMVAE_TENSOR_HIST_BINS 64
#define MMVAE_TENSOR_HIST_STATS 8
/* Host only: the chunk list of a HOST segment table, segments in order, each cut into pieces of at most chunk_elems elements (none for
 * numel = 0).  Returns the number of chunks; writes them when chunks != NULL and capacity (in chunks) suffices, else only counts.
 * -1 (MMVAE_ERR_ARG) for NULL segments, T <= 0, chunk_elems <= 0 or a negative offset / numel. */
MMVAE_API int64_t mmvae_tensor_hist_chunks(const int64_t* segments, int T, int64_t chunk_elems, int64_t* chunks, int64_t capacity);
MMVAE_API size_t mmvae_tensor_hist_scratch_bytes(int T, int64_t n_chunks);
MMVAE_API int mmvae_tensor_hist(const float* flat, int64_t flat_numel, const int64_t* segments, const int64_t* segments_dev, int T,
                                const int64_t* chunks, const int64_t* chunks_dev, int64_t n_chunks, int32_t* counts, float* lo, float* hi,
                                double* stats, void* scratch, size_t scratch_bytes, void* stream);

/* torch.optim.Adam defaults (main.py:468) over a flat buffer: bc1 = 1-beta1^t, bc2_sqrt = sqrt(1-beta2^t);
 * grad_scale multiplies the gradient first (1/world_size after a sum all-reduce). */
MMVAE_API int mmvae_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                    float beta2, float eps, float weight_decay, float bc1, float bc2_sqrt, float grad_scale, void* stream);

/* The same update with the step count on the DEVICE (step_dev[0], a double, incremented by the call; bias corrections are computed
 * from it inside the kernel): the form to capture in a HIP graph -- a captured launch replays its scalar arguments, so the host-side
 * bias corrections of mmvae_adam_step would freeze at the captured step. */
MMVAE_API int mmvae_adam_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                        float beta2, float eps, float weight_decay, double* step_dev, float grad_scale, void* stream);

/* acc[0] += sum_i (grads[i] * grad_scale)^2, every term formed in f64 (the product of two f32 is exact there) and summed like the loss
 * sums above: `partials` is MMVAE_SUM_PARTIALS doubles of scratch (first word zero between calls), NULL runs the sum in one block.
 * `grads` needs no alignment beyond a float's.  The sum is finite exactly when every gradient is: +inf for an inf, NaN for a NaN. */
MMVAE_API int mmvae_grad_norm_sq(const float* grads, int64_t n, float grad_scale, double* acc, double* partials, void* stream);

/* mmvae_adam_step_dev behind two guards, all on the stream (no host read, `grads` is not rewritten; capturable in a HIP graph):
 * the global norm  total = sqrt(mmvae_grad_norm_sq(grads, grad_scale))  is taken first; if it is not finite, params and both
 * moments stay untouched and the step count does not advance; otherwise the gradient is scaled by
 * clip = min(1, max_norm / (total + 1e-6))  (torch.nn.utils.clip_grad_norm_; max_norm <= 0: no clipping, clip = 1) folded with
 * grad_scale into one f32 factor, so a call that does not clip yields the bits of mmvae_adam_step_dev.
 * state (4 doubles, device): [0] step count, incremented by a taken step; [1] total norm of the last call (after grad_scale, before
 * clipping; not finite after a skipped step); [2] number of skipped steps, incremented by a skipped one; [3] the norm^2 accumulator,
 * zero on entry and left at zero.  partials: MMVAE_SUM_PARTIALS doubles as above.  NULL state or partials: MMVAE_ERR_ARG. */
MMVAE_API int mmvae_adam_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                            float beta2, float eps, float weight_decay, double* state, double* partials, float grad_scale,
                            float max_norm, void* stream);

/* ------------------------------------------------------------------ single ops (layer-level parity tests)
 * Conv2d / ConvTranspose2d with PyTorch weight layouts on NHWC activations of `dtype`:
 *   x [N,H,W,Cin], y [N,Ho,Wo,Cout];  weight f32 (Cout,Cin,k,k) for Conv2d, (Cin,Cout,k,k) for ConvTranspose2d.
 * scratch: device buffer of at least 2*numel(weight)*sizeof(dtype)+64 bytes for the packed weights.
 * mmvae_conv2d_fwd with weight == NULL reuses the packed weights an earlier call with the same geometry left in `scratch`.
 * pro_scale/pro_shift (per input channel, nullable): x := relu?(x*scale+shift) applied on load (fused BN+ReLU).
 * stats (nullable): per-channel (sum,sumsq) partials [rows][2][Cout], taken from the f32 accumulators; the call returns `rows`,
 * 1 <= rows <= MMVAE_CONV_STATS_MAX_ROWS (the capacity the caller provides); rows past `rows` are not written.
 * Refused with nothing enqueued and y, stats and scratch untouched: a dtype other than MMVAE_F32 / MMVAE_BF16 (MMVAE_ERR_ARG; the weight
 * gradient entry points below likewise); k*k > 25, Cin no multiple of the 16-byte vector (8 bf16 / 4 f32 channels), Cout no multiple of 4
 * (MMVAE_ERR_UNSUPPORTED). */
#define MMVAE_CONV_STATS_MAX_ROWS 4096
MMVAE_API int mmvae_conv2d_fwd(int dtype, int transposed, const void* x, const float* weight, void* y, int N, int H, int W, int Cin, int Cout,
                     int k, int stride, int pad, const float* pro_scale, const float* pro_shift, int pro_relu, float* stats,
                     void* scratch, void* stream);
/* dx [N,H,W,Cin] from dy [N,Ho,Wo,Cout] */
MMVAE_API int mmvae_conv2d_dgrad(int dtype, int transposed, const void* dy, const float* weight, void* dx, int N, int H, int W, int Cin,
                       int Cout, int k, int stride, int pad, void* scratch, void* stream);
/* The same data gradient with the two options the network's backward pass launches it with (mmvae_conv2d_dgrad is this call with neither,
 * but for bf16 32 -> 32 3x3 stride 1 on 16x16 maps, which it runs as a per-wave stream):
 *   accumulate != 0: dx += (dx must hold valid data of `dtype`) -- the identity blocks' main path onto the shortcut's share;
 *   dy2 / w2 (nullable, both or neither): a second source.  w2 is a Conv2d weight (C2,Cin,1,1) f32 acting on the same input x as the main
 *     layer, and its data gradient is added into dx by the same call (one kernel where the patch-tile kernel merges it, else a second,
 *     accumulating launch):
 *       transposed == 0: the 1x1 conv has the main layer's stride and pad 0 (encoder downsample.0); dy2 [N,Ho,Wo,C2]; its gradient lands on
 *                        stride phase (0,0) of dx.  A stride-2 second source needs even H and W;
 *       transposed == 1: the 1x1 conv has stride 1 (decoder conv1); dy2 [N,H,W,C2], on dx's grid.
 * MMVAE_ERR_ARG, with nothing enqueued and dx untouched: accumulate together with a second source, dy2 without w2 (or w2 without dy2),
 * an odd H or W under a stride-2 second source, a null dy / weight / dx / scratch.
 * scratch: MMVAE_DGRAD_EX_SCRATCH_BYTES(numel(weight), numel(w2), sizeof(dtype)) bytes -- the packed main weights, then (256-byte aligned)
 * the packed w2; with numel(w2) = 0 no more than mmvae_conv2d_dgrad's. */
#define MMVAE_DGRAD_EX_W2_OFFSET(numel_w, esize) ((((size_t)(numel_w) * (esize) + 255) / 256) * 256)
#define MMVAE_DGRAD_EX_SCRATCH_BYTES(numel_w, numel_w2, esize) \
  ((numel_w2) > 0 ? MMVAE_DGRAD_EX_W2_OFFSET(numel_w, esize) + (size_t)(numel_w2) * (esize) : (size_t)(numel_w) * (esize))
MMVAE_API int mmvae_conv2d_dgrad_ex(int dtype, int transposed, const void* dy, const float* weight, void* dx, int N, int H, int W, int Cin,
                          int Cout, int k, int stride, int pad, int accumulate, const void* dy2, const float* w2, int C2, void* scratch,
                          void* stream);
/* dW (f32, weight layout) += ... ; pro_* as in fwd (applied to x).  scratch: MMVAE_WGRAD_SCRATCH_BYTES of device memory
 * (per-block partial images, summed by a second kernel: no atomics, bit-reproducible), owned by the caller.
 * Refused with nothing enqueued, dW and scratch untouched: a NULL scratch (MMVAE_ERR_ARG); k*k > 25, or Cin or Cout no multiple of the
 * 16-byte vector (8 bf16 / 4 f32 channels) (MMVAE_ERR_UNSUPPORTED); and, on the fallback kernel (the shapes no other
 * weight-gradient kernel takes), a weight of Cin*Cout*k*k elements that is no multiple of 256, which the reduce does not take: this needs
 * a channel count that is no multiple of 16 -- bf16 8 -> 8 1x1, f32 4 -> 4 or 4 -> 16 3x3 (MMVAE_ERR_ARG). */
#define MMVAE_WGRAD_SCRATCH_BYTES (64u << 20)
MMVAE_API int mmvae_conv2d_wgrad(int dtype, int transposed, const void* x, const void* dy, float* dweight, int N, int H, int W, int Cin,
                       int Cout, int k, int stride, int pad, const float* pro_scale, const float* pro_shift, int pro_relu,
                       void* scratch, void* stream);
/* Weight gradients of a residual block's conv1 (Conv2d 3x3 stride 2 pad 1) AND of its 1x1 stride-2 shortcut conv from ONE pass over their
 * common input x (encoder.layer1, model.py:29,135-138): dweight [Cout][Cin][3][3] += dy^T (x) x taps, dweight_sc [Cout][Cin][1][1] += dy_sc^T (x) x.
 * bf16, 32 -> 32 channels, 32x32 -> 16x16 (MMVAE_ERR_UNSUPPORTED otherwise); pro_*: BatchNorm+ReLU applied to x on load; scratch as above. */
MMVAE_API int mmvae_conv2d_wgrad_pair(int dtype, const void* x, const void* dy, const void* dy_shortcut, float* dweight, float* dweight_sc, int N,
                            int H, int W, int Cin, int Cout, const float* pro_scale, const float* pro_shift, int pro_relu, void* scratch,
                            void* stream);
/* The forward sibling of mmvae_conv2d_wgrad_pair: a residual block's conv1 (Conv2d 3x3 stride 2 pad 1) AND its 1x1 stride-2 shortcut conv from ONE
 * read of their common input x (what encoder.layer1 runs in a bf16 64x64 step: conv3_stream_kernel with the shortcut's second weight set,
 * second output and second statistics rows).  bf16, 32 -> 32 channels, 32x32 -> 16x16.
 *   y [N,16,16,32] = conv3x3(pro(x), weight (32,32,3,3)), y_sc [N,16,16,32] = conv1x1(pro(x), weight_sc (32,32,1,1)); pro_* as in mmvae_conv2d_fwd
 *   (pro_scale and pro_shift both or neither);
 *   stats, stats_sc (nullable): per-channel (sum, sumsq) partials [rows][2][32] of y and of y_sc, taken from the f32 accumulators.  The call
 *   returns `rows`, 1 <= rows <= MMVAE_FWD_PAIR_MAX_ROWS (the capacity the caller provides for each); a block without work writes a row of zeros;
 *   rows past `rows` are not written.
 * scratch: MMVAE_FWD_PAIR_SCRATCH_BYTES for the packed weights ([cout][tap][cin], then [cout][cin]).
 * Refused with nothing enqueued and y, y_sc, both statistics tensors and scratch untouched: a dtype other than MMVAE_F32 / MMVAE_BF16, a null
 * x / weight / weight_sc / y / y_sc / scratch, pro_scale without pro_shift, N < 1 (MMVAE_ERR_ARG); f32 or any other shape (MMVAE_ERR_UNSUPPORTED). */
#define MMVAE_FWD_PAIR_MAX_ROWS 512
#define MMVAE_FWD_PAIR_SCRATCH_BYTES 20480u
MMVAE_API int mmvae_conv2d_fwd_pair(int dtype, const void* x, const float* weight, const float* weight_sc, void* y, void* y_sc, int N, int H, int W,
                          int Cin, int Cout, const float* pro_scale, const float* pro_shift, int pro_relu, float* stats, float* stats_sc,
                          void* scratch, void* stream);
/* The data gradient of a Conv2d (32,32,3,3) stride 1 pad 1 on 16x16 maps WITH the backward sums of the BatchNorm + ReLU in front of that conv
 * from the same pass (encoder.layer1.conv2's data gradient and bn1's reduce in a bf16 64x64 step):
 *   dx [N,16,16,32] = dgrad(dy [N,16,16,32]), bit for bit mmvae_conv2d_dgrad's on this shape;
 *   sums [rows][2][32] = partial rows of (sum g, sum g * y_pre) per channel, g = dx AS STORED (the bf16-rounded value) where
 *   y_pre * bn_scale + bn_shift > 0 and 0 elsewhere; y_pre [N,16,16,32] is that BatchNorm's input, (bn_scale, bn_shift) its forward coefficients.
 * Returns `rows`, 1 <= rows <= MMVAE_DGRAD_BN_SUMS_MAX_ROWS (the caller's capacity); a block without work writes a row of zeros; rows past
 * `rows` are not written.  scratch: MMVAE_DGRAD_BN_SUMS_SCRATCH_BYTES (the weights packed [cin][flipped tap][cout]).
 * Refused with nothing enqueued and dx, sums and scratch untouched: a dtype other than MMVAE_F32 / MMVAE_BF16, any null pointer, N < 1
 * (MMVAE_ERR_ARG); f32 or H != 16 (MMVAE_ERR_UNSUPPORTED). */
#define MMVAE_DGRAD_BN_SUMS_MAX_ROWS 768
#define MMVAE_DGRAD_BN_SUMS_SCRATCH_BYTES 18432u
MMVAE_API int mmvae_conv2d_dgrad_bn_sums(int dtype, const void* dy, const float* weight, void* dx, const void* y_pre, const float* bn_scale,
                               const float* bn_shift, float* sums, int N, int H, void* scratch, void* stream);
/* ---- BatchNorm2d in training mode and the 1-channel stem, op level (what a maintainer binds instead of torch.nn.BatchNorm2d,
 * model.py:14,20,30,95,..., and of encoder.conv1 + encoder.bn1, model.py:94-95,103)
 * Tensors are NHWC [npix][C] of `dtype`; statistics, parameters and their gradients are f32.
 * scratch: MMVAE_BN_SCRATCH_BYTES of device memory, caller-owned (partial sums of the two-pass reductions, coefficient rows). */
#define MMVAE_BN_SCRATCH_BYTES (16u << 20)
/* out = relu?( (y - mean) * istd * gamma + beta ) with the statistics of this batch (biased variance); running_mean / running_var
 * (nullable) are updated with `momentum` and the unbiased variance, *nbt (nullable) += 1; save_mean / save_istd (C floats each)
 * are kept for the backward pass. */
MMVAE_API int mmvae_batchnorm_fwd(int dtype, const void* y, int64_t npix, int C, const float* gamma, const float* beta, float* running_mean,
                        float* running_var, int64_t* nbt, float momentum, float eps, int relu, void* out, float* save_mean, float* save_istd,
                        void* scratch, void* stream);
/* dy = d(loss)/dy, dgamma += , dbeta += ; dout is the gradient w.r.t. `out`; out (nullable): the forward result when a ReLU was
 * fused (its sign is the mask), NULL for a plain BatchNorm. */
MMVAE_API int mmvae_batchnorm_bwd(int dtype, const void* dout, const void* y, const void* out, int64_t npix, int C, const float* gamma,
                        const float* save_mean, const float* save_istd, void* dy, float* dgamma, float* dbeta, void* scratch, void* stream);
/* encoder.conv1: Conv2d(1 -> 32, k5 s2 p2, no bias) on x [N,S,S] of `dtype` -> y [N,S/2,S/2,32]; stats as mmvae_conv2d_fwd.
 * 9 <= S <= 64.  scratch: MMVAE_STEM_SCRATCH_BYTES for the packed weights -- 32 channels x 25 taps x one 16-byte vector of input channels
 * (8 bf16 / 4 f32, the image in the first): 12 800 bytes in either dtype (bf16 at S = 64 / 32 / 16 builds its weights in registers and
 * leaves the scratch alone). */
#define MMVAE_STEM_SCRATCH_BYTES 12800u
MMVAE_API int mmvae_stem_fwd(int dtype, const void* x, const float* weight, void* y, int N, int S, float* stats, void* scratch, void* stream);
/* Backward of relu(bn(conv1(x))) w.r.t. the parameters in ONE pass over g and y0 (stem_bwd.hip): g = gradient at the block input
 * (post-ReLU activation), y0 = conv1 output, (bn_scale, bn_shift) = gamma*istd, beta - mean*gamma*istd.
 * dweight (32,1,5,5) +=, dgamma +=, dbeta +=.  S in {64, 32, 16}.  scratch: MMVAE_BN_SCRATCH_BYTES. */
MMVAE_API int mmvae_stem_bwd(int dtype, const void* g, const void* y0, const void* x, const float* weight, const float* gamma,
                   const float* bn_scale, const float* bn_shift, const float* save_mean, const float* save_istd, float* dweight,
                   float* dgamma, float* dbeta, int N, int S, void* scratch, void* stream);
/* mmvae_stem_bwd with the incoming gradient never stored: g is recomputed row by row as the data gradient of encoder.layer1's conv1 (Conv2d
 * (32,32,3,3) stride 2 pad 1) plus its 1x1 stride-2 shortcut (32,32,1,1) from their output gradients dy1, dys [N,16,16,32] -- both in one f32
 * accumulator, rounded to bf16 once -- and then treated exactly as mmvae_stem_bwd treats a stored g (what a bf16 64x64 step runs).
 * bf16, S = 64.  The same chain (patch gram, the backward pass, the finalize), the same outputs (dweight +=, dgamma +=, dbeta +=; dgamma and
 * dbeta nullable) and the same scratch carve of MMVAE_BN_SCRATCH_BYTES; its last MMVAE_STEM_DG_PACK_BYTES hold the two packed weights.
 * Refused with nothing enqueued, outputs and scratch untouched: a dtype other than MMVAE_F32 / MMVAE_BF16, a null operand (gamma, dgamma, dbeta
 * excepted), N < 1 (MMVAE_ERR_ARG); f32 or S != 64 (MMVAE_ERR_UNSUPPORTED). */
#define MMVAE_STEM_DG_PACK_BYTES 32768u
MMVAE_API int mmvae_stem_bwd_dg(int dtype, const void* dy1, const void* dys, const float* weight_c1, const float* weight_sc, const void* y0,
                      const void* x, const float* weight, const float* gamma, const float* bn_scale, const float* bn_shift,
                      const float* save_mean, const float* save_istd, float* dweight, float* dgamma, float* dbeta, int N, int S, void* scratch,
                      void* stream);
/* ConvTranspose2d backward in one pass over dy (bf16; Cin = 16 or 32, Cout = 16, k4 s2 p1, 32x32 -> 64x64 or 16x16 -> 32x32; else
 * MMVAE_ERR_UNSUPPORTED):
 * dweight (Cin,Cout,4,4) += , dx [N,H,W,Cin] = d(loss)/dx  (+ x2 (x) w2: x2 [N,H,W,16], w2 f32 (Cin,16,1,1), both nullable).
 * pro_*: as in mmvae_conv2d_wgrad (applied to x).  scratch: (numel(weight) + numel(w2)) * sizeof(dtype) for the packed weights;
 * wscratch: MMVAE_WGRAD_SCRATCH_BYTES.
 * dw2 (nullable, needs x2): the weight gradient of the 1x1 convolution whose data gradient x2 (x) w2 is -- x2 is that conv's output
 * gradient, pro(x) its input -- in the Conv2d layout (16, Cin, 1, 1) (the transpose of w2's (Cin, 16)): dw2 += x2^T (x) pro(x), from the
 * same pass (decoder DeconvBottleneck: conv1's gradient rides on the upsample branch's pass, reference model.py:60,70-72). */
MMVAE_API int mmvae_convT_bwd_fused(int dtype, const void* x, const void* dy, const float* weight, float* dweight, void* dx, int N, int H, int W,
                          int Cin, int Cout, int k, int stride, int pad, const float* pro_scale, const float* pro_shift, int pro_relu,
                          const void* x2, const float* w2, float* dw2, void* scratch, void* wscratch, void* stream);
/* ---- last up-block + tail conv, one output plane (decoder.uplayerN -> decoder.conv2, reference model.py:86-88,193) ----
 * y2, ys: the two branch outputs [N,H,W,16] of `dtype` (BatchNorm not yet applied); (s2,b2), (ss,bs): per-channel f32
 * scale/shift of their BatchNorms; the block output is x = relu(y2*s2+b2 + ys*ss+bs).  weight f32 (1,16,3,3), bias f32 (1).
 * H, W: W a power of two <= 128 (bf16) / 64 (f32), H*W a multiple of that bound; other shapes return MMVAE_ERR_UNSUPPORTED.
 *
 * mmvae_tail_join_fwd: r_raw [N,1,H,W] f32 = conv2d(x, weight, bias, padding=1) without storing x.
 *   stats (nullable): per-image (sum, sumsq) of r_raw, [N][2]; returns N. */
MMVAE_API int mmvae_tail_join_fwd(int dtype, const void* y2, const float* s2, const float* b2, const void* ys, const float* ss, const float* bs,
                        const float* weight, const float* bias, float* r_raw, float* stats, int N, int H, int W, void* stream);
/* The same result as a per-wave MFMA stream (bf16, one output plane, 64x64 only; else MMVAE_ERR_UNSUPPORTED) -- what the network runs:
 * the joined activation and the weights pass through bf16 on their way to the MFMA (mmvae_tail_join_fwd keeps both in f32).
 * stats (nullable): partial (sum, sumsq) rows [rows][2] of r_raw; returns rows (<= N). */
MMVAE_API int mmvae_tail_join_fwd_stream(int dtype, const void* y2, const float* s2, const float* b2, const void* ys, const float* ss, const float* bs,
                               const float* weight, const float* bias, float* r_raw, float* stats, int N, int H, int W, void* stream);
/* mmvae_tail_join_bwd_reduce: with g = conv_transpose2d(d_raw, weight, padding=1) masked by x > 0 (never stored), writes per-block
 *   partial sums partials[rows][3][16] = (sum g, sum g*y2, sum g*ys) and, when wpartials != NULL, the tail conv's weight-gradient
 *   partials wpartials[rows][16][9] (sum over pixels of x[ci] * d_raw[h+1-kh, w+1-kw]); returns rows (<= 1024).
 *   d_raw [N,out_planes,H,W] f32, weight (out_planes,16,3,3); wpartials needs out_planes == 1. */
MMVAE_API int mmvae_tail_join_bwd_reduce(int dtype, const float* d_raw, const float* weight, int out_planes, const void* y2, const float* s2,
                               const float* b2, const void* ys, const float* ss, const float* bs, float* partials, float* wpartials,
                               int N, int H, int W, void* stream);
/* mmvae_tail_join_bwd_apply: dy2 = A2*g + B2*y2 + C2, dys = As*g + Bs*ys + Cs with the same masked g and per-channel f32
 *   coefficient vectors (the BatchNorm-backward affine forms); dy2, dys [N,H,W,16] of `dtype`. */
MMVAE_API int mmvae_tail_join_bwd_apply(int dtype, const float* d_raw, const float* weight, int out_planes, const void* y2, const float* s2,
                              const float* b2, const void* ys, const float* ss, const float* bs, const float* A2, const float* B2,
                              const float* C2, const float* As, const float* Bs, const float* Cs, void* dy2, void* dys, int N, int H, int W,
                              void* stream);
/* ---- the last up-block's backward in ONE pass (conv_joinbwd.hip; bf16, 16 channels, 32x32 -> 64x64, one output plane) ----
 * DeconvBottleneck (reference model.py:70-85) in front of the tail conv (:193): with the join's BatchNorm-backward coefficients at hand
 * (mmvae_tail_join_bwd_reduce + finalize), the kernel produces dy2 / dys row by row in LDS and consumes them in place:
 *   dw_conv2 (16,16,4,4) += a1^T (x) dy2,  d_a1 = conv2's data gradient [N,32,32,16],  bn1_sums[2][16] = (sum g, sum g*y1), g = d_a1 [bn1(y1) > 0]
 *   dw_up    (16,16,4,4) += pro(xin)^T (x) dys,  g_in = the upsample branch's data gradient [N,32,32,16]   (conv1's share: mmvae_conv1x1_bwd_fused)
 * y1: conv2's input before bn1 (s1, b1 = bn1's scale / shift, ReLU); xin: the block input (sx, bx: optional BatchNorm+ReLU in front, nullable).
 * Nothing of size dy2 / dys is written.  scratch: MMVAE_WGRAD_SCRATCH_BYTES (packed weights, partial images). */
MMVAE_API int mmvae_upblock_bwd_fused(const float* d_raw, const float* tail_weight, const void* y2, const float* s2, const float* b2,
                            const void* ys, const float* ss, const float* bs, const float* A2, const float* B2, const float* C2,
                            const float* As, const float* Bs, const float* Cs, const void* y1, const float* s1, const float* b1,
                            const float* w_conv2, float* dw_conv2, void* d_a1, float* bn1_sums, const void* xin, const float* sx,
                            const float* bx, const float* w_up, float* dw_up, void* g_in, int N, void* scratch, void* stream);
/* conv1 (1x1, 16 -> 16) of the same block, once bn1's sums are final (A1, B1, C1 = its backward coefficients):
 *   dy1 = A1 (d_a1 [bn1(y1) > 0]) + B1 y1 + C1;  g_in += dy1 (x) W1 (in place);  dw_conv1 (16,16,1,1) += dy1^T (x) pro(xin).
 * rows = N * H rows of 32 pixels.  scratch: MMVAE_WGRAD_SCRATCH_BYTES. */
/* The same block's FORWARD tail: r_raw = decoder.conv2(relu(bn2(conv2(relu(bn1(y1)))) + upsample.1(upsample.0(x_in)))) (model.py:70-85,193) with both
 * ConvTranspose2d branch outputs recomputed row by row from their 32x32x16 inputs instead of read back (this call does not write them: see
 * mmvae_upblock_tail_fwd_store).  bf16 NHWC inputs, f32 weights in PyTorch layout (w2, wu: [16][16][4][4]; tail
 * weight [1][16][3][3] + bias), s / b pairs = forward scale / shift of the BatchNorms (sx / bx may be NULL: x_in is an activation);
 * r_raw f32 [N][64][64]; stats (nullable) receives <return value> partial rows [2] = (sum, sum of squares) of r_raw; scratch >= 16 KB. */
MMVAE_API int mmvae_upblock_tail_fwd(const void* y1, const float* s1, const float* b1, const float* w2, const void* x_in, const float* sx,
                                     const float* bx, const float* wu, const float* s2, const float* b2, const float* ss, const float* bs,
                                     const float* tail_weight, const float* tail_bias, float* r_raw, float* stats, int N, void* scratch,
                                     void* stream);
/* The same launch, also STORING the two branch outputs the backward pass reads: y2 = conv2(relu(bn1(y1))), ys = upsample.0(x_in), both
 * [N][64][64][16] bf16 and bit-identical to what mmvae_conv2d_fwd writes for the same inputs (the same f32 accumulators, the same rounding).
 * r_raw and stats are those of mmvae_upblock_tail_fwd bit for bit.  y2 and ys are both required here. */
MMVAE_API int mmvae_upblock_tail_fwd_store(const void* y1, const float* s1, const float* b1, const float* w2, const void* x_in, const float* sx,
                                           const float* bx, const float* wu, const float* s2, const float* b2, const float* ss, const float* bs,
                                           const float* tail_weight, const float* tail_bias, float* r_raw, float* stats, void* y2, void* ys,
                                           int N, void* scratch, void* stream);
/* The batch statistics of ConvTranspose2d(16 -> 16, k4 s2 p1) on x [N][32][32][16] WITHOUT its output (what the training step runs in front of
 * mmvae_upblock_tail_fwd_store): stats receives <return value> partial rows [2][16], bit-identical to those of mmvae_conv2d_fwd on the
 * same inputs; pro_scale / pro_shift (both or neither) as there, with ReLU.  dtype: bf16 only; e4m3_out != 0 (the fp8 storage mode has
 * no such form) and other dtypes are refused.  weight (16,16,4,4) f32; scratch >= 8 KB for the packed weights. */
MMVAE_API int mmvae_convT4_stats(int dtype, const void* x, const float* weight, const float* pro_scale, const float* pro_shift, float* stats,
                                 int N, int e4m3_out, void* scratch, void* stream);
/* A block's residual join fused with the NEXT block's conv1 (reference model.py:86-88 of block i, :72 of block i + 1; conv_joinfwd.hip; bf16):
 *   out = relu(s2 y2 + b2 + ss ys + bs)  [npix][C]  (C = 16 or 32; written: the upsample branch and the backward pass read it),
 *   y1 = conv1(out), w_conv1 (16, C, 1, 1) f32, no bias, [npix][16];  stats (nullable): <return value> partial rows [2][16] = (sum, sum of
 *   squares) of y1 from the f32 accumulators.  npix a multiple of 32; scratch >= 2 KB (the packed weight). */
MMVAE_API int mmvae_join_conv1x1_fwd(const void* y2, const float* s2, const float* b2, const void* ys, const float* ss, const float* bs,
                           const float* w_conv1, int C, void* out, void* y1, float* stats, int64_t npix, void* scratch, void* stream);
MMVAE_API int mmvae_conv1x1_bwd_fused(const void* d_a1, const void* y1, const float* s1, const float* b1, const float* A1, const float* B1,
                            const float* C1, const void* xin, const float* sx, const float* bx, const float* w_conv1, float* dw_conv1,
                            void* g_in, int64_t rows, void* scratch, void* stream);
/* ------------------------------------------------------------------ PixelCNN (reference model.py:212-255)
 * PixelCNN(in_channels, intermediate_channels, out_channels, layers, "ReLu"):  InstanceNorm2d -> [MaskedConv2d('A' first, then 'B', 7x7 pad 3,
 * bias) -> InstanceNorm2d -> ReLU] x (layers - 1) -> MaskedConv2d('B').  The masks (model.py:216-220) keep the first 24 ('A') / 25 ('B') taps
 * of the 7x7 kernel in row-major order: the layers run as convolutions over exactly those taps, so a masked tap's stored weight is never
 * read and its gradient is left untouched (the reference zeroes the tap before every use, model.py:222).
 * params / grads: flat f32, per layer weight (out, in, 7, 7) then bias (out) -- the reference's parameter order.  x, d_x: [N,in,S,S] f32;
 * out, d_out: [N,out,S,S] f32 logits.  in / out channels <= 16, intermediate_channels a multiple of 16 in [16, 256], 2 <= layers <= 16;
 * dtype f32 or bf16 (storage of the activations between the layers).  mmvae_pixelcnn_bwd needs the workspace of the forward it
 * differentiates and that forward's x. */
typedef struct mmvae_pixelcnn mmvae_pixelcnn;
MMVAE_API int mmvae_pixelcnn_create(mmvae_pixelcnn** out, int in_channels, int intermediate_channels, int out_channels, int layers, int dtype);
MMVAE_API void mmvae_pixelcnn_destroy(mmvae_pixelcnn* net);
MMVAE_API int64_t mmvae_pixelcnn_num_params(mmvae_pixelcnn* net);
MMVAE_API size_t mmvae_pixelcnn_workspace_bytes(mmvae_pixelcnn* net, int N, int S);
MMVAE_API int mmvae_pixelcnn_fwd(mmvae_pixelcnn* net, int N, int S, const float* x, const float* params, void* workspace, size_t workspace_bytes,
                       float* out, void* stream);
MMVAE_API int mmvae_pixelcnn_bwd(mmvae_pixelcnn* net, int N, int S, const float* x, const float* d_out, const float* params, float* grads,
                       void* workspace, size_t workspace_bytes, float* d_x, void* stream);
/* Autoregressive sampling (reference main.py:186-202): the whole S x S loop enqueued on `stream`, no host synchronisation.  The net's input is
 * cond [N, cond_channels, S, S] f32 (the decoder image of a PixelVAE; NULL with 0 channels) followed by sample [N, sample_channels, S, S] f32;
 * cond_channels + sample_channels must equal the net's in_channels.  For pixel p = i * S + j in row-major order: layers 0 .. layers - 2 run over
 * the full map (their InstanceNorms see every pixel, so nothing is cached), the last layer is evaluated at pixel p only, and
 *   label = #{k in [0, out_channels - 2] : cdf_k <= uniforms[n][p]},  cdf = cumulative sums of softmax(logits) in channel order (f32),
 *   sample[n, c, i, j] = (label - sub_mean) / data_std for every sample channel c
 * (the distribution of torch.multinomial(probs, 1), from the caller's uniforms in [0, 1)).  The reference's PixelCNN-only loop passes
 * sub_mean = 0, its PixelVAE loop the data mean.  Optional outputs (NULL: not written): out_logits [N, out, S, S] = the full forward on the sample
 * as it was before the last pixel was written (what the reference's loop returns), probs [N, S*S, out] f32 and labels [N, S*S] of each draw.
 * Errors (nothing is enqueued): channel counts, data_std == 0, NULL uniforms / sample: MMVAE_ERR_ARG; workspace too small: MMVAE_ERR_WORKSPACE.
 * The workspace may be the forward's; a sampling call overwrites what mmvae_pixelcnn_bwd needs. */
MMVAE_API size_t mmvae_pixelcnn_sample_workspace_bytes(mmvae_pixelcnn* net, int N, int S);
MMVAE_API int mmvae_pixelcnn_sample(mmvae_pixelcnn* net, int N, int S, const float* cond, int cond_channels, float* sample, int sample_channels,
                          const float* uniforms, float sub_mean, float data_std, const float* params, void* workspace, size_t workspace_bytes,
                          float* out_logits, float* probs, int64_t* labels, void* stream);

/* f32 <-> dtype element conversion (n elements) */
MMVAE_API int mmvae_convert(int dtype_in, int dtype_out, const void* in, void* out, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMVAE_H_ */

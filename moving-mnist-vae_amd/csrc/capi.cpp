// extern "C" surface declared in include/mmvae.h.
#include <cstring>
#include <new>

#include "../../include/mmvae.h"
#include "conv_ops.hpp"
#include "pixel_net.hpp"
#include "quantiser_fit.hpp"
#include "resample.hpp"
#include "vae_net.hpp"

namespace mmvae { const char* last_error(); }
using namespace mmvae;

struct mmvae_net { Net* net; };
struct mmvae_comm { Comm* c; };

static inline hipStream_t stream_of(void* s) { return static_cast<hipStream_t>(s); }

extern "C" {

int mmvae_abi_version(void) { return MMVAE_ABI_VERSION; }
const char* mmvae_last_error(void) { return last_error(); }

int mmvae_net_create(mmvae_net** out, int in_channels, int z, int out_channels, int image_size, int need_logvar, int dtype) {
  return mmvae_net_create_ex(out, in_channels, z, out_channels, image_size, need_logvar, dtype, 1);
}
int mmvae_net_create_ex(mmvae_net** out, int in_channels, int z, int out_channels, int image_size, int need_logvar, int dtype,
                        int blocks_per_stage) {
  if (!out) return MMVAE_ERR_ARG;
  if (blocks_per_stage < 1 || blocks_per_stage > 4) { set_error("blocks_per_stage=%d unsupported (1..4)", blocks_per_stage); return MMVAE_ERR_UNSUPPORTED; }
  if (in_channels < 1 || in_channels > 4) { set_error("in_channels=%d unsupported (1..4; the benchmarked path is the 1-channel Moving-MNIST VAE)", in_channels); return MMVAE_ERR_UNSUPPORTED; }
  if (z <= 0 || z % 8) { set_error("z_dimension=%d must be a positive multiple of 8", z); return MMVAE_ERR_UNSUPPORTED; }
  if (!(out_channels == 1 || out_channels == 2 || out_channels == 3 || out_channels == 4 || out_channels == 8)) {
    set_error("decoder_out_channels=%d unsupported (1,2,3,4,8)", out_channels); return MMVAE_ERR_UNSUPPORTED; }
  if (image_size < 9 || image_size > 64) { set_error("input_image_size=%d unsupported (9..64)", image_size); return MMVAE_ERR_UNSUPPORTED; }
  if (dtype != MMVAE_F32 && dtype != MMVAE_BF16 && dtype != MMVAE_FP8) { set_error("dtype=%d unsupported", dtype); return MMVAE_ERR_ARG; }
  // MMVAE_FP8: bf16 storage everywhere, fp8 (e4m3) MFMA in the forward pass of the deep layers
  NetCfg c{in_channels, z, out_channels, image_size, need_logvar ? 1 : 0, dtype == MMVAE_FP8 ? MMVAE_BF16 : dtype, blocks_per_stage, dtype == MMVAE_FP8 ? 1 : 0};
  mmvae_net* h = new (std::nothrow) mmvae_net;
  if (!h) return MMVAE_ERR_ARG;
  h->net = new (std::nothrow) Net(c);
  if (!h->net) { delete h; return MMVAE_ERR_ARG; }
  *out = h;
  return MMVAE_OK;
}
void mmvae_net_destroy(mmvae_net* n) { if (n) { delete n->net; delete n; } }

int mmvae_net_sizes(const mmvae_net* n, int64_t* n_params, int64_t* n_bn_f32, int32_t* n_bn_i64, int64_t* dec_off, int32_t* dec_side) {
  if (!n) return MMVAE_ERR_ARG;
  if (n_params) *n_params = n->net->n_params;
  if (n_bn_f32) *n_bn_f32 = n->net->n_bnbuf;
  if (n_bn_i64) *n_bn_i64 = n->net->n_nbt;
  if (dec_off) *dec_off = n->net->dec_param_off;
  if (dec_side) *dec_side = n->net->Sd;
  return MMVAE_OK;
}
int mmvae_net_num_entries(const mmvae_net* n) { return n ? (int)n->net->entries.size() : MMVAE_ERR_ARG; }
int mmvae_net_entry(const mmvae_net* n, int i, char* name, int cap, int32_t* ndim, int32_t shape[4], int32_t* kind, int64_t* offset) {
  if (!n || i < 0 || i >= (int)n->net->entries.size()) return MMVAE_ERR_ARG;
  const Entry& e = n->net->entries[i];
  if (name && cap > 0) { std::strncpy(name, e.name.c_str(), cap - 1); name[cap - 1] = 0; }
  if (ndim) *ndim = e.ndim;
  if (shape) for (int k = 0; k < 4; ++k) shape[k] = e.shape[k];
  if (kind) *kind = e.kind;
  if (offset) *offset = e.offset;
  return MMVAE_OK;
}
size_t mmvae_net_workspace_bytes(mmvae_net* n, int N) { return n && N > 0 ? n->net->workspace_bytes(N) : 0; }

int mmvae_encoder_fwd(mmvae_net* n, int N, const float* x, const float* params, float* bn_f32, int64_t* bn_i64, void* ws, size_t wsb,
                      float* mu, float* logvar, int training, void* stream) {
  if (!n || N <= 0 || !x || !params || !ws || !mu) { set_error("encoder_fwd: bad argument"); return MMVAE_ERR_ARG; }
  if (n->net->cfg.need_logvar && !logvar) { set_error("encoder_fwd: logvar required"); return MMVAE_ERR_ARG; }
  if (!bn_f32) { set_error("encoder_fwd: BN buffers required"); return MMVAE_ERR_ARG; }
  return n->net->encoder_fwd(N, x, params, bn_f32, reinterpret_cast<long long*>(bn_i64), ws, wsb, mu, logvar, training, stream_of(stream));
}
int mmvae_net_stage_labels(mmvae_net* n, int N, const void* labels, int label_bytes, float mean, float stdv, float* image, void* ws, size_t wsb,
                           void* stream) {
  if (!n || N <= 0 || !labels || !image || !ws) { set_error("net_stage_labels: bad argument"); return MMVAE_ERR_ARG; }
  return n->net->stage_labels(N, labels, label_bytes, mean, stdv, image, ws, wsb, stream_of(stream));
}
int mmvae_encoder_fwd_staged(mmvae_net* n, int N, const float* x, const float* params, float* bn_f32, int64_t* bn_i64, void* ws, size_t wsb,
                             float* mu, float* logvar, int training, void* stream) {
  if (!n || N <= 0 || !x || !params || !ws || !mu) { set_error("encoder_fwd_staged: bad argument"); return MMVAE_ERR_ARG; }
  if (n->net->cfg.need_logvar && !logvar) { set_error("encoder_fwd_staged: logvar required"); return MMVAE_ERR_ARG; }
  if (!bn_f32) { set_error("encoder_fwd_staged: BN buffers required"); return MMVAE_ERR_ARG; }
  return n->net->encoder_fwd(N, x, params, bn_f32, reinterpret_cast<long long*>(bn_i64), ws, wsb, mu, logvar, training, stream_of(stream), true);
}
int mmvae_encoder_bwd(mmvae_net* n, int N, const float* d_mu, const float* d_logvar, const float* params, float* grads, void* ws,
                      size_t wsb, void* stream) {
  if (!n || N <= 0 || !d_mu || !params || !grads || !ws) { set_error("encoder_bwd: bad argument"); return MMVAE_ERR_ARG; }
  if (n->net->cfg.need_logvar && !d_logvar) { set_error("encoder_bwd: d_logvar required"); return MMVAE_ERR_ARG; }
  return n->net->encoder_bwd(N, d_mu, d_logvar, params, grads, ws, wsb, stream_of(stream));
}
int mmvae_decoder_fwd(mmvae_net* n, int N, const float* enc, const float* params, float* bn_f32, int64_t* bn_i64, void* ws, size_t wsb,
                      float* recon, int training, void* stream) {
  if (!n || N <= 0 || !enc || !params || !ws || !recon || !bn_f32) { set_error("decoder_fwd: bad argument"); return MMVAE_ERR_ARG; }
  return n->net->decoder_fwd(N, enc, params, bn_f32, reinterpret_cast<long long*>(bn_i64), ws, wsb, recon, training, stream_of(stream));
}
int mmvae_decoder_bwd(mmvae_net* n, int N, const float* d_recon, const float* params, float* grads, void* ws, size_t wsb, float* d_enc,
                      void* stream) {
  if (!n || N <= 0 || !d_recon || !params || !grads || !ws) { set_error("decoder_bwd: bad argument"); return MMVAE_ERR_ARG; }
  return n->net->decoder_bwd(N, d_recon, params, grads, ws, wsb, d_enc, stream_of(stream));
}

int mmvae_decoder_bwd_gauss(mmvae_net* n, int N, const float* target, float sigma, float coef, const float* gscale, const float* params, float* grads,
                            void* ws, size_t wsb, float* d_enc, void* stream) {
  if (!n || N <= 0 || !target || !params || !grads || !ws || !(sigma > 0.f)) { set_error("decoder_bwd_gauss: bad argument"); return MMVAE_ERR_ARG; }
  const Net::GaussTail gt{target, sigma, coef, gscale};
  return n->net->decoder_bwd(N, nullptr, params, grads, ws, wsb, d_enc, stream_of(stream), &gt);
}

int mmvae_net_defer_join(mmvae_net* n, int enable) {
  if (!n) { set_error("net_defer_join: bad argument"); return MMVAE_ERR_ARG; }
  n->net->set_defer_join(enable != 0);
  return MMVAE_OK;
}
int mmvae_net_join(mmvae_net* n, void* stream) {
  if (!n) { set_error("net_join: bad argument"); return MMVAE_ERR_ARG; }
  return n->net->join(stream_of(stream));
}

void* mmvae_net_fork(mmvae_net* n, void* stream) {
  if (!n) return stream;
  return reinterpret_cast<void*>(n->net->fork(stream_of(stream)));
}

int mmvae_net_set_join_grad(mmvae_net* n, int enable) {
  if (!n) { set_error("net_set_join_grad: bad argument"); return MMVAE_ERR_ARG; }
  n->net->set_join_grad(enable != 0);
  return MMVAE_OK;
}

int mmvae_net_describe_routes(mmvae_net* n, int N, char* buf, int cap) {
  if (!n || N <= 0 || cap < 0 || (!buf && cap > 0)) { set_error("net_describe_routes: bad argument"); return MMVAE_ERR_ARG; }
  std::string text;
  const int rc = n->net->describe_routes(N, text);
  if (rc < 0) return rc;
  if (cap > 0) { std::strncpy(buf, text.c_str(), cap - 1); buf[cap - 1] = 0; }
  return (int)text.size() + 1;
}

void* mmvae_net_side_stream(mmvae_net* n) { return n ? reinterpret_cast<void*>(n->net->side()) : nullptr; }

int mmvae_net_set_sync_bn(mmvae_net* n, mmvae_allreduce_fn fn, void* user, int world) {
  if (!n || (fn && world < 1)) { set_error("net_set_sync_bn: bad argument"); return MMVAE_ERR_ARG; }
  n->net->set_sync_bn(reinterpret_cast<mmvae::Net::AllReduceFn>(fn), user, world);
  return MMVAE_OK;
}

// ---- data-parallel exchange
int mmvae_comm_unique_id(void* id) {
  if (!id) { set_error("comm_unique_id: bad argument"); return MMVAE_ERR_ARG; }
  return comm_unique_id(id);
}
int mmvae_comm_init(mmvae_comm** out, int world, int rank, const void* id) {
  if (!out || !id || world < 1 || rank < 0 || rank >= world) { set_error("comm_init: bad argument"); return MMVAE_ERR_ARG; }
  mmvae_comm* h = new (std::nothrow) mmvae_comm;
  if (!h) return MMVAE_ERR_ARG;
  h->c = nullptr;
  const int rc = comm_init(&h->c, world, rank, id);
  if (rc < 0) { delete h; return rc; }
  *out = h;
  return MMVAE_OK;
}
int mmvae_comm_allreduce(mmvae_comm* c, float* buf, int64_t n, void* st) {
  if (!c || (!buf && n > 0)) { set_error("comm_allreduce: bad argument"); return MMVAE_ERR_ARG; }
  return comm_allreduce_sum(c->c, buf, (long long)n, stream_of(st));
}
int mmvae_comm_destroy(mmvae_comm* c) {
  if (!c) return MMVAE_OK;
  const int rc = comm_destroy(c->c);
  delete c;
  return rc;
}
int mmvae_net_set_sync_bn_comm(mmvae_net* n, mmvae_comm* c) {
  if (!n) { set_error("net_set_sync_bn_comm: bad argument"); return MMVAE_ERR_ARG; }
  n->net->set_sync_bn_comm(c ? c->c : nullptr);
  return MMVAE_OK;
}
int mmvae_net_set_sync_bn_comm2(mmvae_net* n, mmvae_comm* cm, mmvae_comm* cs) {
  if (!n || (!cm && cs)) { set_error("net_set_sync_bn_comm2: bad argument"); return MMVAE_ERR_ARG; }
  n->net->set_sync_bn_comm(cm ? cm->c : nullptr, cs ? cs->c : nullptr);
  return MMVAE_OK;
}

// ---- PixelCNN (reference model.py:212-255)
struct mmvae_pixelcnn { PixelNet* net; };
int mmvae_pixelcnn_create(mmvae_pixelcnn** out, int in_channels, int intermediate_channels, int out_channels, int layers, int dtype) {
  if (!out) { set_error("pixelcnn_create: bad argument"); return MMVAE_ERR_ARG; }
  if (dtype != MMVAE_F32 && dtype != MMVAE_BF16) { set_error("pixelcnn_create: dtype must be f32 or bf16"); return MMVAE_ERR_UNSUPPORTED; }
  if (in_channels < 1 || in_channels > 16 || out_channels < 1 || out_channels > 16 || layers < 2 || layers > 16 || intermediate_channels < 16 ||
      intermediate_channels > 256 || intermediate_channels % 16) {
    set_error("pixelcnn_create: unsupported shape (in %d, intermediate %d, out %d, layers %d): in / out <= 16, intermediate a multiple of 16 in [16, 256], "
              "2 <= layers <= 16", in_channels, intermediate_channels, out_channels, layers);
    return MMVAE_ERR_UNSUPPORTED;
  }
  mmvae_pixelcnn* h = new (std::nothrow) mmvae_pixelcnn;
  if (!h) return MMVAE_ERR_ARG;
  h->net = new PixelNet(in_channels, intermediate_channels, out_channels, layers, dtype == MMVAE_F32 ? DT_F32 : DT_BF16);
  *out = h;
  return MMVAE_OK;
}
void mmvae_pixelcnn_destroy(mmvae_pixelcnn* h) { if (h) { delete h->net; delete h; } }
int64_t mmvae_pixelcnn_num_params(mmvae_pixelcnn* h) { return h ? (int64_t)h->net->n_params : -1; }
size_t mmvae_pixelcnn_workspace_bytes(mmvae_pixelcnn* h, int N, int S) { return (h && N > 0 && S > 0) ? h->net->workspace_bytes(N, S) : 0; }
int mmvae_pixelcnn_fwd(mmvae_pixelcnn* h, int N, int S, const float* x, const float* params, void* ws, size_t wsb, float* out, void* st) {
  if (!h || N <= 0 || S <= 0 || !x || !params || !ws || !out) { set_error("pixelcnn_fwd: bad argument"); return MMVAE_ERR_ARG; }
  return h->net->forward(N, S, x, params, ws, wsb, out, stream_of(st));
}
int mmvae_pixelcnn_bwd(mmvae_pixelcnn* h, int N, int S, const float* x, const float* d_out, const float* params, float* grads, void* ws, size_t wsb,
                       float* d_x, void* st) {
  if (!h || N <= 0 || S <= 0 || !x || !d_out || !params || !grads || !ws) { set_error("pixelcnn_bwd: bad argument"); return MMVAE_ERR_ARG; }
  return h->net->backward(N, S, x, d_out, params, grads, ws, wsb, d_x, stream_of(st));
}
size_t mmvae_pixelcnn_sample_workspace_bytes(mmvae_pixelcnn* h, int N, int S) { return mmvae_pixelcnn_workspace_bytes(h, N, S); }
int mmvae_pixelcnn_sample(mmvae_pixelcnn* h, int N, int S, const float* cond, int cond_channels, float* sample, int sample_channels,
                          const float* uniforms, float sub_mean, float data_std, const float* params, void* ws, size_t wsb, float* out_logits,
                          float* probs, int64_t* labels, void* st) {
  if (!h || N <= 0 || S <= 0 || !sample || !uniforms || !params || !ws) { set_error("pixelcnn_sample: bad argument"); return MMVAE_ERR_ARG; }
  return h->net->sample(N, S, cond, cond_channels, sample, sample_channels, uniforms, sub_mean, data_std, params, ws, wsb, out_logits, probs,
                        reinterpret_cast<long long*>(labels), stream_of(st));
}

// ---- latent / loss
int mmvae_rsample_fwd(const float* mu, const float* lv, const float* eps, float* enc, int64_t n, void* st) {
  return launch_rsample_fwd(DT_F32, mu, lv, eps, enc, nullptr, (long)n, stream_of(st));
}
int mmvae_rsample_bwd(const float* d_enc, const float* lv, const float* eps, float* d_mu, float* d_lv, int64_t n, void* st) {
  return launch_rsample_bwd(d_enc, lv, eps, d_mu, d_lv, (long)n, stream_of(st));
}
static bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }
// The loss sums: *_ex takes the ordered-reduction scratch (required); the plain form passes none and runs the sum in one block.
int mmvae_kl_fwd_ex(const float* mu, const float* lv, int64_t n, double* acc, double* partials, void* st) {
  if (n > 0 && (!mu || !lv || !acc || !partials)) { set_error("kl_fwd: bad argument"); return MMVAE_ERR_ARG; }
  return launch_kl_fwd(mu, lv, (long)n, acc, partials, stream_of(st));
}
int mmvae_kl_fwd(const float* mu, const float* lv, int64_t n, double* acc, void* st) {
  if (n > 0 && (!mu || !lv || !acc)) { set_error("kl_fwd: bad argument"); return MMVAE_ERR_ARG; }
  return launch_kl_fwd(mu, lv, (long)n, acc, nullptr, stream_of(st));
}
int mmvae_kl_bwd(const float* mu, const float* lv, float coef, const float* gscale, float* d_mu, float* d_lv, int64_t n, void* st) {
  return launch_kl_bwd(mu, lv, coef, gscale, d_mu, d_lv, (long)n, stream_of(st));
}
static int gauss_nll_fwd(const float* r, const float* t, int64_t n, float sigma, double* acc, double* partials, bool need_partials, void* st) {
  if (!(sigma > 0.f)) { set_error("gauss_nll: sigma must be > 0"); return MMVAE_ERR_ARG; }
  if (n > 0 && (!r || !t || !acc || (need_partials && !partials))) { set_error("gauss_nll_fwd: bad argument"); return MMVAE_ERR_ARG; }
  if (n > 0 && (!aligned16(r) || !aligned16(t))) { set_error("gauss_nll_fwd: recon and target must be 16-byte aligned"); return MMVAE_ERR_ARG; }
  return launch_gauss_nll_fwd(r, t, (long)n, sigma, acc, partials, stream_of(st));
}
int mmvae_gauss_nll_fwd_ex(const float* r, const float* t, int64_t n, float sigma, double* acc, double* partials, void* st) {
  return gauss_nll_fwd(r, t, n, sigma, acc, partials, true, st);
}
int mmvae_gauss_nll_fwd(const float* r, const float* t, int64_t n, float sigma, double* acc, void* st) {
  return gauss_nll_fwd(r, t, n, sigma, acc, nullptr, false, st);
}
int mmvae_gauss_nll_bwd(const float* r, const float* t, int64_t n, float sigma, float coef, const float* gscale, float* d_r, void* st) {
  if (!(sigma > 0.f)) { set_error("gauss_nll: sigma must be > 0"); return MMVAE_ERR_ARG; }
  return launch_gauss_nll_bwd(r, t, (long)n, sigma, coef, gscale, d_r, stream_of(st));
}
int mmvae_ce_fwd_ex(const float* r, const int64_t* t, const float* w, int N, int Q, int HW, double* acc, double* partials, void* st) {
  if ((long)N * HW > 0 && (!r || !t || !acc || !partials || Q < 1)) { set_error("ce_fwd: bad argument"); return MMVAE_ERR_ARG; }
  return launch_ce_fwd(r, reinterpret_cast<const long long*>(t), w, N, Q, HW, acc, partials, stream_of(st));
}
int mmvae_ce_fwd(const float* r, const int64_t* t, const float* w, int N, int Q, int HW, double* acc, void* st) {
  if ((long)N * HW > 0 && (!r || !t || !acc || Q < 1)) { set_error("ce_fwd: bad argument"); return MMVAE_ERR_ARG; }
  return launch_ce_fwd(r, reinterpret_cast<const long long*>(t), w, N, Q, HW, acc, nullptr, stream_of(st));
}
int mmvae_ce_bwd(const float* r, const int64_t* t, const float* w, int N, int Q, int HW, float coef, const float* gscale, float* d_r,
                 void* st) {
  return launch_ce_bwd(r, reinterpret_cast<const long long*>(t), w, N, Q, HW, coef, gscale, d_r, stream_of(st));
}
static int mmd_fwd(const float* x, const float* y, int n, int d, float* scratch, double* acc, double* partials, bool need_partials, void* st) {
  if (n > 0 && (!x || !y || !acc || (need_partials && !partials) || d < 1)) { set_error("mmd_fwd: bad argument"); return MMVAE_ERR_ARG; }
  if (n > 0 && scratch && (!aligned16(x) || !aligned16(y))) { set_error("mmd_fwd: x and y must be 16-byte aligned"); return MMVAE_ERR_ARG; }
  return scratch ? launch_mmd_fwd_mfma(x, y, n, d, scratch, acc, partials, stream_of(st)) : launch_mmd_fwd(x, y, n, d, acc, partials, stream_of(st));
}
int mmvae_mmd_fwd_ex(const float* x, const float* y, int n, int d, float* scratch, double* acc, double* partials, void* st) {
  return mmd_fwd(x, y, n, d, scratch, acc, partials, true, st);
}
int mmvae_mmd_fwd(const float* x, const float* y, int n, int d, float* scratch, double* acc, void* st) {
  return mmd_fwd(x, y, n, d, scratch, acc, nullptr, false, st);
}
int mmvae_mmd_bwd(const float* x, const float* y, int n, int d, float coef, const float* gscale, float* d_y, void* st) {
  return launch_mmd_bwd(x, y, n, d, coef, gscale, d_y, stream_of(st));
}
int mmvae_rbf_kernel(const float* x, const float* y, int n, int m, int d, float* out, void* st) {
  if (!x || !y || !out) { set_error("rbf_kernel: bad argument"); return MMVAE_ERR_ARG; }
  return launch_rbf_matrix(x, y, n, m, d, out, stream_of(st));
}
int mmvae_loss_finish(const double* acc, float* out, float nll, float kl_coef, float mmd_coef, float n, void* st) {
  return launch_loss_finish(acc, out, nll, kl_coef, mmd_coef, n, stream_of(st));
}

// ---- held-out evaluation: per-image f64 terms (eval_loss.hip).  A bad argument returns before anything is enqueued.
int mmvae_gauss_nll_per_image(const float* r, const float* t, int N, int64_t per, float sigma, double* out, void* st) {
  if (!(sigma > 0.f)) { set_error("gauss_nll_per_image: sigma must be > 0"); return MMVAE_ERR_ARG; }
  if (!r || !t || !out || N < 1 || per < 1) { set_error("gauss_nll_per_image: bad argument"); return MMVAE_ERR_ARG; }
  return launch_gauss_nll_per_image(r, t, N, (long)per, sigma, out, stream_of(st));
}
int mmvae_ce_per_image(const float* r, const int64_t* t, const float* w, int N, int Q, int HW, double* out, void* st) {
  if (!r || !t || !out || N < 1 || Q < 1 || HW < 1) { set_error("ce_per_image: bad argument"); return MMVAE_ERR_ARG; }
  return launch_ce_per_image(r, reinterpret_cast<const long long*>(t), w, N, Q, HW, out, stream_of(st));
}
int mmvae_kl_per_image(const float* mu, const float* lv, int N, int d, double* out, void* st) {
  if (!mu || !lv || !out || N < 1 || d < 1) { set_error("kl_per_image: bad argument"); return MMVAE_ERR_ARG; }
  return launch_kl_per_image(mu, lv, N, d, out, stream_of(st));
}
int mmvae_latent_logratio(const float* mu, const float* lv, const float* eps, int N, int d, double* out, void* st) {
  if (!mu || !lv || !eps || !out || N < 1 || d < 1) { set_error("latent_logratio: bad argument"); return MMVAE_ERR_ARG; }
  return launch_latent_logratio(mu, lv, eps, N, d, out, stream_of(st));
}
int mmvae_iw_bound(const double* nll, const double* logratio, int K, int N, double* out, void* st) {
  if (!nll || !logratio || !out || K < 1 || N < 1) { set_error("iw_bound: bad argument"); return MMVAE_ERR_ARG; }
  return launch_iw_bound(nll, logratio, K, N, out, stream_of(st));
}

// ---- plumbing
int mmvae_normalise_labels(const int64_t* labels, int64_t n, float mean, float stdv, float* image, void* st) {
  return launch_normalise(DT_F32, labels, 8, (long)n, mean, stdv, nullptr, image, stream_of(st));
}
int mmvae_quantise_normalise(const uint8_t* frames, int64_t n, const float* centres, int q, float mean, float stdv, int64_t* labels,
                             float* image, void* st) {
  return launch_quantise_normalise(frames, (long)n, centres, q, mean, stdv, reinterpret_cast<long long*>(labels), image, stream_of(st));
}
int mmvae_u8_histogram(const uint8_t* frames, int64_t clip_bytes, const int64_t* clip_index, int64_t n_clips, uint64_t* counts, void* st) {
  return launch_u8_histogram(frames, (long)clip_bytes, reinterpret_cast<const long long*>(clip_index), (long)n_clips,
                             reinterpret_cast<unsigned long long*>(counts), stream_of(st));
}
int mmvae_kmeans1d_fit(const uint64_t* counts, int q, double* centres, double* inertia) { return kmeans1d_fit(counts, q, centres, inertia); }
int mmvae_quantiser_stats(const uint64_t* counts, const float* centres, int q, uint8_t* lut, double* ratios, double* label_mean,
                          double* label_std) {
  return quantiser_stats(counts, centres, q, lut, ratios, label_mean, label_std);
}
int mmvae_resample_coeffs(int in_size, int out_size, int* ksize, int32_t* bounds, int32_t* coeffs) {
  return resample_coeffs(in_size, out_size, ksize, bounds, coeffs);
}
int mmvae_resize_quantise_normalise(const uint8_t* frames, int64_t frame_stride_bytes, const int64_t* clip_index, int frames_per_clip,
                                    int64_t n_frames, int in_h, int in_w, int out_h, int out_w, const int32_t* h_bounds,
                                    const int32_t* h_coeffs, int h_ksize, const int32_t* v_bounds, const int32_t* v_coeffs, int v_ksize,
                                    const float* centres, int q, float mean, float stdv, int64_t* labels, float* image, uint8_t* resized,
                                    void* st) {
  return launch_resize_quantise_normalise(frames, (long)frame_stride_bytes, reinterpret_cast<const long long*>(clip_index), frames_per_clip,
                                          (long)n_frames, in_h, in_w, out_h, out_w, h_bounds, h_coeffs, h_ksize, v_bounds, v_coeffs, v_ksize,
                                          centres, q, mean, stdv, reinterpret_cast<long long*>(labels), image, resized, stream_of(st));
}
int mmvae_generate_clips(const uint8_t* bank, int64_t D, int G, const int32_t* vel, uint64_t seed, int64_t first_clip, int64_t n_clips, int T,
                         int S, int K, const float* centres, int q, float mean, float stdv, int64_t* labels, float* image, uint8_t* bytes,
                         void* st) {
  return launch_generate_clips(bank, (long)D, G, vel, (unsigned long long)seed, (long)first_clip, (long)n_clips, T, S, K, centres, q, mean,
                               stdv, reinterpret_cast<long long*>(labels), image, bytes, stream_of(st));
}
// ---- picture panels (pointers and ranges are checked in the launchers, before anything is enqueued)
int mmvae_logits_to_labels(const float* logits, int N, int Q, int HW, int mode, const float* uniforms, int64_t* labels, void* st) {
  return launch_logits_to_labels(logits, N, Q, HW, mode, uniforms, reinterpret_cast<long long*>(labels), stream_of(st));
}
int mmvae_panel_sheet(const mmvae_panel_col* cols, int ncols, int n, int S, uint8_t* out, void* st) {
  return launch_panel_sheet(cols, ncols, n, S, out, stream_of(st));
}
int mmvae_frame_quality(const mmvae_panel_col* a, const mmvae_panel_col* b, int n, int S, double* out, void* st) {
  return launch_frame_quality(a, b, n, S, out, stream_of(st));
}
// ---- latent diagnostics (arguments are checked in the launchers)
int mmvae_scatter_panel(const float* pts, int64_t n, int stride, int col_x, int col_y, const float* xform, int side, int radius16,
                        const uint8_t* tone, uint8_t* out, int64_t out_row_stride, void* st) {
  return launch_scatter_panel(pts, (long)n, stride, col_x, col_y, xform, side, radius16, tone, out, (long)out_row_stride, stream_of(st));
}
int mmvae_latent_stats(const float* mu, const float* logvar, const float* enc, int N, int d, int accumulate, double* acc, void* st) {
  return launch_latent_stats(mu, logvar, enc, N, d, accumulate, acc, stream_of(st));
}
// ---- aggregate-posterior densities (arguments are checked in the launcher)
size_t mmvae_posterior_mixture_scratch_bytes(int N, int M, int d) { return posterior_mixture_scratch_bytes(N, M, d); }
int mmvae_posterior_mixture(const float* z, int N, const float* mu, const float* logvar, int M, int d, double* log_qz, double* log_qz_dims,
                            void* scratch, size_t scratch_bytes, void* st) {
  return launch_posterior_mixture(z, N, mu, logvar, M, d, log_qz, log_qz_dims, scratch, scratch_bytes, stream_of(st));
}
size_t mmvae_posterior_mixture_bwd_scratch_bytes(int N, int M, int d) { return posterior_mixture_bwd_scratch_bytes(N, M, d); }
int mmvae_posterior_mixture_bwd(const float* z, int N, const float* mu, const float* logvar, int M, int d, const double* log_qz,
                                const double* log_qz_dims, const double* g_joint, const double* g_dims, float* d_z, float* d_mu,
                                float* d_logvar, void* scratch, size_t scratch_bytes, void* st) {
  return launch_posterior_mixture_bwd(z, N, mu, logvar, M, d, log_qz, log_qz_dims, g_joint, g_dims, d_z, d_mu, d_logvar, scratch, scratch_bytes,
                                      stream_of(st));
}
// ---- nearest training frames (arguments are checked in the launcher)
size_t mmvae_nearest_frames_scratch_bytes(int M, int64_t F, int D, int k) { return nearest_frames_scratch_bytes(M, (long)F, D, k); }
int mmvae_nearest_frames(const uint8_t* queries, int M, const uint8_t* frames, int64_t F, int D, const uint8_t* lut, int k, int32_t* out_dist,
                         int64_t* out_index, void* scratch, size_t scratch_bytes, void* st) {
  return launch_nearest_frames(queries, M, frames, (long)F, D, lut, k, out_dist, reinterpret_cast<long long*>(out_index), scratch, scratch_bytes,
                               stream_of(st));
}
// ---- set-to-set k-NN and ball counts (arguments are checked in the launcher)
size_t mmvae_knn_cross_scratch_bytes(int64_t Na, int64_t Nb, int D, int k, int want_count) {
  return knn_cross_scratch_bytes((long)Na, (long)Nb, D, k, want_count);
}
int mmvae_knn_cross(const uint8_t* a, int64_t Na, const uint8_t* b, int64_t Nb, int D, int k, int exclude_diagonal, int32_t* out_dist,
                    int64_t* out_index, const int32_t* col_radius, int32_t* out_count, void* scratch, size_t scratch_bytes, void* st) {
  return launch_knn_cross(a, (long)Na, b, (long)Nb, D, k, exclude_diagonal, out_dist, reinterpret_cast<long long*>(out_index), col_radius,
                          out_count, scratch, scratch_bytes, stream_of(st));
}
// ---- per-tensor histograms of a flat buffer (arguments are checked in the launcher)
int64_t mmvae_tensor_hist_chunks(const int64_t* segments, int T, int64_t chunk_elems, int64_t* chunks, int64_t capacity) {
  return tensor_hist_chunks(reinterpret_cast<const long long*>(segments), T, (long long)chunk_elems, reinterpret_cast<long long*>(chunks),
                            (long long)capacity);
}
size_t mmvae_tensor_hist_scratch_bytes(int T, int64_t n_chunks) { return tensor_hist_scratch_bytes(T, (long long)n_chunks); }
int mmvae_tensor_hist(const float* flat, int64_t flat_numel, const int64_t* segments, const int64_t* segments_dev, int T, const int64_t* chunks,
                      const int64_t* chunks_dev, int64_t n_chunks, int32_t* counts, float* lo, float* hi, double* stats, void* scratch,
                      size_t scratch_bytes, void* st) {
  return launch_tensor_hist(flat, (long long)flat_numel, reinterpret_cast<const long long*>(segments),
                            reinterpret_cast<const long long*>(segments_dev), T, reinterpret_cast<const long long*>(chunks),
                            reinterpret_cast<const long long*>(chunks_dev), (long long)n_chunks, counts, lo, hi, stats, scratch, scratch_bytes,
                            stream_of(st));
}
int mmvae_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, float wd, float bc1,
                    float bc2_sqrt, float grad_scale, void* st) {
  AdamArgs a{p, g, m, v, (long)n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, grad_scale};
  return launch_adam(a, stream_of(st));
}

int mmvae_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, float wd,
                        double* step_dev, float grad_scale, void* st) {
  if (!step_dev) { set_error("adam_step_dev: step counter required"); return MMVAE_ERR_ARG; }
  AdamArgs a{p, g, m, v, (long)n, lr, b1, b2, eps, wd, 1.f, 1.f, grad_scale};
  return launch_adam_dev(a, step_dev, stream_of(st));
}

int mmvae_grad_norm_sq(const float* g, int64_t n, float grad_scale, double* acc, double* partials, void* st) {
  if (n > 0 && (!g || !acc)) { set_error("grad_norm_sq: bad argument"); return MMVAE_ERR_ARG; }
  return launch_grad_norm_sq(g, (long)n, grad_scale, acc, partials, stream_of(st));
}

int mmvae_adam_step_guarded(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, float wd,
                            double* state, double* partials, float grad_scale, float max_norm, void* st) {
  if (n > 0 && (!p || !g || !m || !v)) { set_error("adam_step_guarded: bad argument"); return MMVAE_ERR_ARG; }
  if (n > 0 && (!state || !partials)) { set_error("adam_step_guarded: state and partials required"); return MMVAE_ERR_ARG; }
  AdamArgs a{p, g, m, v, (long)n, lr, b1, b2, eps, wd, 1.f, 1.f, grad_scale};
  return launch_adam_guarded(a, state, partials, max_norm, stream_of(st));
}

// ---- single ops
static inline ConvGeom geom_for(int transposed, int Cin, int Cout, int k, int s, int p) {
  // Conv2d weight (Cout,Cin,k,k): D0=Cout (small side = y), D1=Cin.  ConvT weight (Cin,Cout,k,k): D0=Cin (small side = x), D1=Cout.
  return transposed ? ConvGeom{Cin, Cout, k, s, p} : ConvGeom{Cout, Cin, k, s, p};
}
static inline long numel_w(int Cin, int Cout, int k) { return (long)Cin * Cout * k * k; }
static inline int out_size(int transposed, int H, int k, int s, int p) { return transposed ? (H - 1) * s - 2 * p + k : conv_down_size(H, k, s, p); }
// Refusals of the single-op conv entry points, asked before anything is enqueued.  The dtype: anything that is not f32 used to run as bf16.
static_assert(MMVAE_CONV_STATS_MAX_ROWS >= kGatherMaxGridX * kMaxPhases, "statistics rows: one per block and stride phase");
static int conv_dtype_refused(const char* who, int dt) {
  if (dt == MMVAE_F32 || dt == MMVAE_BF16) return MMVAE_OK;
  set_error("%s: dtype=%d unsupported", who, dt);
  return MMVAE_ERR_ARG;
}
// launch_gather_gemm's own conditions, which the forward would otherwise only reach after its packing launch
static int conv_fwd_refused(int dt, int Cin, int Cout, int k) {
  if (const int rc = conv_dtype_refused("conv2d_fwd", dt); rc < 0) return rc;
  const int ve = dt == MMVAE_F32 ? 4 : 8;
  if (k < 1 || k * k > kMaxTaps) { set_error("conv2d_fwd: k=%d unsupported (at most %d taps)", k, kMaxTaps); return MMVAE_ERR_UNSUPPORTED; }
  if (Cin < 1 || Cout < 1 || Cin % ve != 0 || Cout % 4 != 0) {
    set_error("conv2d_fwd: unsupported Cin=%d Cout=%d (Cin a multiple of %d, Cout of 4)", Cin, Cout, ve); return MMVAE_ERR_UNSUPPORTED;
  }
  return MMVAE_OK;
}

int mmvae_conv2d_fwd(int dt, int transposed, const void* x, const float* w, void* y, int N, int H, int W, int Cin, int Cout, int k,
                     int s, int p, const float* ps, const float* pb, int relu, float* stats, void* scratch, void* st) {
  if (const int rc = conv_fwd_refused(dt, Cin, Cout, k); rc < 0) return rc;
  const ConvGeom g = geom_for(transposed, Cin, Cout, k, s, p);
  const int Ho = out_size(transposed, H, k, s, p), Wo = out_size(transposed, W, k, s, p);
  const MapIn in(x, H, W, Affine{ps, pb}, relu);
  const MapOut out(y, Ho, Wo, stats);
  // weight == NULL: `scratch` still holds the packed weights of an earlier call with the same geometry (pack once, run many)
  SecondSrc q;
  if (!transposed && conv3_stream_ok(dt, Cin, Cout, k, s, p, H, W)) {      // the first encoder block's 3x3 convs: per-wave stream
    if (w) { int rc = op_pack_down(dt, g, w, scratch, stream_of(st)); if (rc < 0) return rc; }
    return launch_conv3_stream(dt, s, in, scratch, nullptr, out, MapOut(), N, stream_of(st));
  }
  if (!transposed) {
    q.wfrag = op_down_layout(dt, g, H, W).frag;
    if (w) { int rc = op_pack_down(dt, g, w, scratch, stream_of(st), 1.f, 0, q.wfrag); if (rc < 0) return rc; }
    return op_run_down(dt, dt, g, scratch, in, out, N, stream_of(st), q);
  }
  if (convT4_stream_ok(dt, Cin, Cout, k, s, p, H, W)) {                   // the decoder's widest ConvT layers: per-wave stream
    if (w) { int rc = op_pack_up(dt, g, w, scratch, stream_of(st)); if (rc < 0) return rc; }
    return launch_convT4_stream(dt, in, scratch, out, N, stream_of(st));
  }
  q.wfrag = op_up_layout(dt, g, Ho, Wo).frag;
  if (w) { int rc = op_pack_up(dt, g, w, scratch, stream_of(st), 1.f, 0, q.wfrag); if (rc < 0) return rc; }
  return op_run_up(dt, g, scratch, in, out, N, stream_of(st), q);
}
int mmvae_conv2d_dgrad(int dt, int transposed, const void* dy, const float* w, void* dx, int N, int H, int W, int Cin, int Cout, int k,
                       int s, int p, void* scratch, void* st) {
  if (!transposed && s == 1 && conv3_stream_ok(dt, Cin, Cout, k, s, p, H, W)) {
    // encoder.layer1.conv2's shape: the data gradient as a forward conv over dy with the weights packed [cin][flipped tap][cout] (op_pack_flipped3)
    int rc = op_pack_flipped3(dt, w, scratch, Cin, Cout, stream_of(st)); if (rc < 0) return rc;
    rc = launch_conv3_stream(dt, 1, MapIn(dy, H, W), scratch, nullptr, MapOut(dx, H, W), MapOut(), N, stream_of(st));
    return rc < 0 ? rc : MMVAE_OK;
  }
  // everything else: the launch Net::run_up / Net::run_down make, with neither option
  return mmvae_conv2d_dgrad_ex(dt, transposed, dy, w, dx, N, H, W, Cin, Cout, k, s, p, 0, nullptr, nullptr, 0, scratch, st);
}
// The data-gradient launches of Net::run_up / Net::run_down with their two options: accumulate (the identity blocks' main path onto the
// shortcut's share) and the second source (the 1x1 branch of a residual join, riding along or as its own accumulating launch).  Layouts as
// Net::settle_layout settles them.  (No per-wave stream form here: the network takes that one through launch_conv3_stream_bwd, never
// through run_up.)  Every refusal returns before anything is enqueued.
int mmvae_conv2d_dgrad_ex(int dt, int transposed, const void* dy, const float* w, void* dx, int N, int H, int W, int Cin, int Cout, int k,
                          int s, int p, int accumulate, const void* dy2, const float* w2, int C2, void* scratch, void* st) {
  if (dt != MMVAE_F32 && dt != MMVAE_BF16) { set_error("conv2d_dgrad: dtype=%d unsupported", dt); return MMVAE_ERR_ARG; }
  if (!dy || !w || !dx || !scratch || N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || k < 1 || s < 1 || p < 0) {
    set_error("conv2d_dgrad: bad argument"); return MMVAE_ERR_ARG;
  }
  if ((dy2 != nullptr) != (w2 != nullptr)) { set_error("conv2d_dgrad: dy2 and w2 go together"); return MMVAE_ERR_ARG; }
  if (dy2 && accumulate) { set_error("conv2d_dgrad: accumulate with a second source is not a launch of the network"); return MMVAE_ERR_ARG; }
  if (dy2 && C2 < 1) { set_error("conv2d_dgrad: C2=%d", C2); return MMVAE_ERR_ARG; }
  if (dy2 && !transposed && s == 2 && ((H | W) & 1)) {
    set_error("conv2d_dgrad: a stride-2 second source needs even H and W (%d x %d): its phase (0, 0) is the q grid", H, W); return MMVAE_ERR_ARG;
  }
  const ConvGeom g = geom_for(transposed, Cin, Cout, k, s, p);
  const int Ho = out_size(transposed, H, k, s, p), Wo = out_size(transposed, W, k, s, p);
  char* sc = static_cast<char*>(scratch);
  const MapIn in(dy, Ho, Wo);
  const MapOut out(dx, H, W, nullptr, accumulate != 0);
  SecondSrc q;
  if (dy2) {
    // Conv2d (C2, Cin, 1, 1) on the main layer's input: with the main Conv2d's stride (encoder downsample.0), stride 1 beside a ConvTranspose2d
    // (decoder conv1).  Its data gradient is an up launch on dx's grid either way; packed behind the main weights.
    const ConvGeom g2 = geom_for(0, Cin, C2, 1, transposed ? 1 : s, 0);
    q.wfrag2 = op_up_layout(dt, g2, H, W, 1).frag;
    void* w2p = sc + MMVAE_DGRAD_EX_W2_OFFSET(numel_w(Cin, Cout, k), dtype_size(dt));
    int rc = op_pack_up(dt, g2, w2, w2p, stream_of(st), 1.f, 0, q.wfrag2); if (rc < 0) return rc;
    q.x2 = dy2; q.w2 = w2p; q.Cin2 = C2;
  }
  if (!transposed) {
    q.wfrag = op_up_layout(dt, g, H, W, accumulate != 0).frag;
    int rc = op_pack_up(dt, g, w, scratch, stream_of(st), 1.f, 0, q.wfrag); if (rc < 0) return rc;
    return op_run_up(dt, g, scratch, in, out, N, stream_of(st), q);
  }
  q.wfrag = op_down_layout(dt, g, Ho, Wo).frag;
  int rc = op_pack_down(dt, g, w, scratch, stream_of(st), 1.f, 0, q.wfrag); if (rc < 0) return rc;
  return op_run_down(dt, dt, g, scratch, in, out, N, stream_of(st), q);
}
int mmvae_conv2d_wgrad(int dt, int transposed, const void* x, const void* dy, float* dw, int N, int H, int W, int Cin, int Cout, int k,
                       int s, int p, const float* ps, const float* pb, int relu, void* scratch, void* st) {
  const ConvGeom g = geom_for(transposed, Cin, Cout, k, s, p);
  const int Ho = out_size(transposed, H, k, s, p), Wo = out_size(transposed, W, k, s, p);
  if (!scratch) { set_error("conv2d_wgrad: scratch (MMVAE_WGRAD_SCRATCH_BYTES) required"); return MMVAE_ERR_ARG; }
  if (const int rc = conv_dtype_refused("conv2d_wgrad", dt); rc < 0) return rc;
  static_assert(MMVAE_WGRAD_SCRATCH_BYTES == kWgradScratchBytes, "public scratch size out of sync");
  WgradOpts o;
  o.scratch = static_cast<float*>(scratch);
  const MapIn in(x, H, W, Affine{ps, pb}, relu), grad(dy, Ho, Wo);
  if (!transposed) return op_run_wgrad(dt, g, grad, in, dw, N, stream_of(st), o);
  return op_run_wgrad(dt, g, in, grad, dw, N, stream_of(st), o);
}
int mmvae_conv2d_wgrad_pair(int dt, const void* x, const void* dy, const void* dy_sc, float* dw, float* dw_sc, int N, int H, int W, int Cin, int Cout,
                            const float* ps, const float* pb, int relu, void* scratch, void* st) {
  if (!scratch || !x || !dy || !dy_sc || !dw || !dw_sc || N < 1) { set_error("conv2d_wgrad_pair: bad argument"); return MMVAE_ERR_ARG; }
  if (const int rc = conv_dtype_refused("conv2d_wgrad_pair", dt); rc < 0) return rc;
  const ConvGeom g = geom_for(0, Cin, Cout, 3, 2, 1), gs = geom_for(0, Cin, Cout, 1, 2, 0);
  const int Ho = out_size(0, H, 3, 2, 1), Wo = out_size(0, W, 3, 2, 1);
  WgradOpts o;
  o.scratch = static_cast<float*>(scratch);
  const int rc = op_run_wgrad_pair(dt, g, gs, MapIn(dy, Ho, Wo), dy_sc, MapIn(x, H, W, Affine{ps, pb}, relu), dw, dw_sc, N, stream_of(st), o);
  if (rc == 0) { set_error("conv2d_wgrad_pair: shape not supported (bf16, 32 -> 32 channels, 32x32 -> 16x16)"); return MMVAE_ERR_UNSUPPORTED; }
  return rc < 0 ? rc : MMVAE_OK;
}
// ---- the encoder-entry kernels of a bf16 64x64 training step, each as the launches Net::encoder_fwd / Net::encoder_bwd make around
// encoder.layer1.  Every refusal returns before anything is enqueued (the packing launches included).
static_assert(MMVAE_FWD_PAIR_SCRATCH_BYTES >= (32 * 9 * 32 + 32 * 32) * 2, "pair scratch: the [cout][tap][cin] and the [32][32] pack");
static_assert(MMVAE_DGRAD_BN_SUMS_SCRATCH_BYTES >= 32 * 9 * 32 * 2, "dgrad scratch: the [cin][flipped tap][cout] pack");
int mmvae_conv2d_fwd_pair(int dt, const void* x, const float* w, const float* w_sc, void* y, void* y_sc, int N, int H, int W, int Cin, int Cout,
                          const float* ps, const float* pb, int relu, float* stats, float* stats_sc, void* scratch, void* st) {
  if (const int rc = conv_dtype_refused("conv2d_fwd_pair", dt); rc < 0) return rc;
  if (!x || !w || !w_sc || !y || !y_sc || !scratch || N < 1 || (ps != nullptr) != (pb != nullptr)) {
    set_error("conv2d_fwd_pair: bad argument (x, both weights, both outputs and scratch required; pro_scale and pro_shift go together)");
    return MMVAE_ERR_ARG;
  }
  if (!conv3_stream_ok(dt, Cin, Cout, 3, 2, 1, H, W)) {
    set_error("conv2d_fwd_pair: shape not supported (bf16, 32 -> 32 channels, 32x32 -> 16x16)"); return MMVAE_ERR_UNSUPPORTED;
  }
  char* sc = static_cast<char*>(scratch);
  void* wsp = sc + (size_t)32 * 9 * 32 * dtype_size(dt);
  int rc = op_pack_down(dt, geom_for(0, Cin, Cout, 3, 2, 1), w, sc, stream_of(st)); if (rc < 0) return rc;
  rc = op_pack_down(dt, geom_for(0, Cin, Cout, 1, 2, 0), w_sc, wsp, stream_of(st)); if (rc < 0) return rc;
  return launch_conv3_stream(dt, 2, MapIn(x, H, W, Affine{ps, pb}, relu), sc, wsp, MapOut(y, H / 2, W / 2, stats), MapOut(y_sc, H / 2, W / 2, stats_sc), N,
                             stream_of(st));
}
int mmvae_conv2d_dgrad_bn_sums(int dt, const void* dy, const float* w, void* dx, const void* y_pre, const float* bn_scale, const float* bn_shift,
                               float* sums, int N, int H, void* scratch, void* st) {
  if (const int rc = conv_dtype_refused("conv2d_dgrad_bn_sums", dt); rc < 0) return rc;
  if (!dy || !w || !dx || !y_pre || !bn_scale || !bn_shift || !sums || !scratch || N < 1) {
    set_error("conv2d_dgrad_bn_sums: bad argument (every operand and scratch required, N >= 1)"); return MMVAE_ERR_ARG;
  }
  if (dt != MMVAE_BF16 || H != 16) { set_error("conv2d_dgrad_bn_sums: shape not supported (bf16, 32 -> 32 channels, 16x16 maps)"); return MMVAE_ERR_UNSUPPORTED; }
  int rc = op_pack_flipped3(dt, w, scratch, 32, 32, stream_of(st)); if (rc < 0) return rc;
  return launch_conv3_stream_bwd(dt, MapIn(dy, H, H), scratch, BnSide{y_pre, {bn_scale, bn_shift}}, MapOut(dx, H, H, sums), N, stream_of(st));
}
int mmvae_convT_bwd_fused(int dt, const void* x, const void* dy, const float* w, float* dw, void* dx, int N, int H, int W, int Cin, int Cout, int k,
                          int s, int p, const float* ps, const float* pb, int relu, const void* x2, const float* w2, float* dw2, void* scratch,
                          void* wscratch, void* st) {
  const ConvGeom g = geom_for(1, Cin, Cout, k, s, p);
  const int Ho = out_size(1, H, k, s, p), Wo = out_size(1, W, k, s, p);
  if (!scratch || !wscratch) { set_error("convT_bwd_fused: scratch buffers required"); return MMVAE_ERR_ARG; }
  if (const int rc = conv_dtype_refused("convT_bwd_fused", dt); rc < 0) return rc;
  if (!op_bwd_fusable(dt, g, MapIn::shape(H, W), MapIn::shape(Ho, Wo), N)) { set_error("convT_bwd_fused: shape not supported (bf16, 16 / 32 -> 16 channels, k4 s2 p1, 32x32 -> 64x64 or 16x16 -> 32x32)"); return MMVAE_ERR_UNSUPPORTED; }
  char* sc = static_cast<char*>(scratch);
  int rc = op_pack_down(dt, g, w, sc, stream_of(st)); if (rc < 0) return rc;
  const void* w2p = nullptr;
  if (x2 && w2) {
    PackArgs pa; std::memset(&pa, 0, sizeof(pa));
    pa.src = w2; pa.dst = sc + (size_t)Cin * Cout * k * k * dtype_size(dt); pa.cols = Cin; pa.K = 16; pa.ntaps = 1; pa.s_col = 16; pa.s_k = 1; pa.scale = 1.f; pa.tap_off[0] = 0;
    rc = launch_pack(dt, pa, stream_of(st)); if (rc < 0) return rc;
    w2p = pa.dst;
  }
  if (dw2 && !w2p) { set_error("convT_bwd_fused: dw2 needs x2 and w2"); return MMVAE_ERR_ARG; }
  SecondSrc q;
  if (w2p) { q.x2 = x2; q.w2 = w2p; }
  WgradOpts o;
  o.scratch = static_cast<float*>(wscratch); o.dW2 = dw2;
  rc = op_run_bwd_fused(dt, g, sc, MapIn(x, H, W, Affine{ps, pb}, relu), MapIn(dy, Ho, Wo), q, dx, dw, N, stream_of(st), o);
  if (rc == 0) { set_error("convT_bwd_fused: not taken"); return MMVAE_ERR_UNSUPPORTED; }
  return rc < 0 ? rc : MMVAE_OK;
}
// ---- op-level BatchNorm / stem (compositions of the kernels the network orchestrator launches)
static_assert(MMVAE_BN_SCRATCH_BYTES >= (1024u * 3 * 512 + 8 * 512) * 4, "BatchNorm scratch: 1024 partial rows x 3 x C<=512 + coefficient rows");
int mmvae_batchnorm_fwd(int dt, const void* y, int64_t npix, int C, const float* gamma, const float* beta, float* rm, float* rv, int64_t* nbt,
                        float momentum, float eps, int relu, void* out, float* save_mean, float* save_istd, void* scratch, void* st) {
  if (!scratch || !save_mean || !save_istd || C < 1 || C > 512 || npix < 1) { set_error("batchnorm_fwd: bad arguments (C <= 512, scratch and save_* required)"); return MMVAE_ERR_ARG; }
  float* part = static_cast<float*>(scratch);
  float* coef = part + 1024L * 3 * 512;              // scale, shift
  const int np = launch_chan_stats_nhwc(dt, y, npix, C, part, stream_of(st));
  if (np < 0) return np;
  BnFinalizeArgs f;
  f.partials = part; f.nparts = np; f.C = C; f.count = (double)npix; f.gamma = gamma; f.beta = beta; f.running_mean = rm; f.running_var = rv;
  f.nbt = reinterpret_cast<long long*>(nbt); f.mean = save_mean; f.istd = save_istd; f.scale = coef; f.shift = coef + C; f.momentum = momentum; f.eps = eps;
  int rc = launch_bn_finalize(f, stream_of(st));
  if (rc < 0) return rc;
  return launch_affine_act(dt, BnSide{y, {coef, coef + C}}, relu, out, npix, C, stream_of(st));
}
int mmvae_batchnorm_bwd(int dt, const void* dout, const void* y, const void* out, int64_t npix, int C, const float* gamma, const float* save_mean,
                        const float* save_istd, void* dy, float* dgamma, float* dbeta, void* scratch, void* st) {
  if (!scratch || C < 1 || C > 512 || npix < 1) { set_error("batchnorm_bwd: bad arguments (C <= 512, scratch required)"); return MMVAE_ERR_ARG; }
  float* part = static_cast<float*>(scratch);
  float* coef = part + 1024L * 3 * 512;              // A, B, C
  const BnSide side{y, {}, {coef, coef + C, coef + 2 * C}};
  const int np = launch_bn_bwd_reduce(dt, dout, out, side, BnSide{}, part, npix, C, stream_of(st));
  if (np < 0) return np;
  BnBwdFinalizeArgs f; std::memset(&f, 0, sizeof(f));
  f.partials = part; f.nparts = np; f.C = C; f.which = 0; f.ny = 1; f.count = (double)npix; f.gamma = gamma; f.mean = save_mean; f.istd = save_istd;
  f.dgamma = dgamma; f.dbeta = dbeta; f.coefA = coef; f.coefB = coef + C; f.coefC = coef + 2 * C;
  int rc = launch_bn_bwd_finalize(f, stream_of(st));
  if (rc < 0) return rc;
  return launch_bn_bwd_apply(dt, dout, out, side, BnSide{}, dy, nullptr, npix, C, stream_of(st));
}
static_assert(MMVAE_STEM_SCRATCH_BYTES >= 32 * 25 * 16, "stem scratch: 32 columns x 25 taps x one 16-byte vector of padded input channels");
int mmvae_stem_fwd(int dt, const void* x, const float* w, void* y, int N, int Sz, float* stats, void* scratch, void* st) {
  if (!scratch || N < 1 || Sz < 9 || Sz > 64) { set_error("stem_fwd: bad arguments"); return MMVAE_ERR_ARG; }
  if (stem_fwd_stream_ok(dt, Sz)) return launch_stem_fwd_stream(dt, x, w, y, stats, N, Sz, stream_of(st));
  const int H1 = conv_down_size(Sz, 5, 2, 2);
  const int rc = op_pack_stem(dt, w, 1, scratch, stream_of(st));
  if (rc < 0) return rc;
  return op_run_stem(dt, scratch, x, 1, Sz, MapOut(y, H1, H1, stats), N, stream_of(st));
}
int mmvae_stem_bwd(int dt, const void* g, const void* y0, const void* x, const float* w, const float* gamma, const float* bn_scale,
                   const float* bn_shift, const float* save_mean, const float* save_istd, float* dw, float* dgamma, float* dbeta, int N, int Sz,
                   void* scratch, void* st) {
  if (!scratch || N < 1) { set_error("stem_bwd: bad arguments"); return MMVAE_ERR_ARG; }
  if (!stem_bwd_fusable(Sz)) { set_error("stem_bwd: image size %d unsupported (64, 32, 16)", Sz); return MMVAE_ERR_UNSUPPORTED; }
  const int H1 = (Sz + 4 - 5) / 2 + 1;
  // carve: R (1024 doubles) | gram partials (1024 x part floats) | backward partials (the rest)
  double* R = static_cast<double*>(scratch);
  float* gram = reinterpret_cast<float*>(R + 1024);
  const long gram_floats = 1024L * stem_bwd_part_floats();
  float* part = gram + gram_floats;
  const long part_floats = (long)(MMVAE_BN_SCRATCH_BYTES - 1024 * 8) / 4 - gram_floats;
  int rc = launch_stem_gram(dt, x, gram, gram_floats, R, N, Sz, H1, H1, stream_of(st));
  if (rc < 0) return rc;
  const int np = launch_stem_bwd(dt, g, y0, x, bn_scale, bn_shift, part, part_floats, N, Sz, H1, H1, stream_of(st));
  if (np < 0) return np;
  return launch_stem_bwd_finalize(part, np, R, w, nullptr, (double)N * H1 * H1, gamma, save_mean, save_istd, dgamma, dbeta, dw, stream_of(st));
}
// mmvae_stem_bwd's chain with the incoming gradient recomputed from encoder.layer1's dy tensors (launch_stem_bwd_dg): the same carve, the two
// transposed-form weight packs (op_pack_up, no fragment order: what Net::packs_enc_bwd leaves for this kernel) in the scratch's last 32 KB
static_assert(MMVAE_STEM_DG_PACK_BYTES >= (32 * 9 * 32 + 32 * 32) * 2 && MMVAE_STEM_DG_PACK_BYTES % 256 == 0, "stem DG packs");
int mmvae_stem_bwd_dg(int dt, const void* dy1, const void* dys, const float* w_c1, const float* w_sc, const void* y0, const void* x, const float* w,
                      const float* gamma, const float* bn_scale, const float* bn_shift, const float* save_mean, const float* save_istd, float* dw,
                      float* dgamma, float* dbeta, int N, int Sz, void* scratch, void* st) {
  if (const int rc = conv_dtype_refused("stem_bwd_dg", dt); rc < 0) return rc;
  if (!dy1 || !dys || !w_c1 || !w_sc || !y0 || !x || !w || !bn_scale || !bn_shift || !save_mean || !save_istd || !dw || !scratch || N < 1) {
    set_error("stem_bwd_dg: bad argument (every operand but gamma, dgamma, dbeta required; N >= 1)"); return MMVAE_ERR_ARG;
  }
  if (!stem_bwd_dg_ok(dt, Sz)) { set_error("stem_bwd_dg: bf16 and image size 64 only (dtype=%d, S=%d)", dt, Sz); return MMVAE_ERR_UNSUPPORTED; }
  const int H1 = Sz / 2;
  double* R = static_cast<double*>(scratch);
  float* gram = reinterpret_cast<float*>(R + 1024);
  const long gram_floats = 1024L * stem_bwd_part_floats();
  float* part = gram + gram_floats;
  const long part_floats = (long)(MMVAE_BN_SCRATCH_BYTES - MMVAE_STEM_DG_PACK_BYTES - 1024 * 8) / 4 - gram_floats;
  static_assert((MMVAE_BN_SCRATCH_BYTES - MMVAE_STEM_DG_PACK_BYTES - 1024 * 8) / 4 - 1024L * (64 + 32 * 32) >= 768L * (64 + 32 * 32), "768 partial rows fit");
  char* pk1 = static_cast<char*>(scratch) + (MMVAE_BN_SCRATCH_BYTES - MMVAE_STEM_DG_PACK_BYTES);
  char* pks = pk1 + (size_t)32 * 9 * 32 * dtype_size(dt);
  int rc = op_pack_up(dt, geom_for(0, 32, 32, 3, 2, 1), w_c1, pk1, stream_of(st)); if (rc < 0) return rc;
  rc = op_pack_up(dt, geom_for(0, 32, 32, 1, 2, 0), w_sc, pks, stream_of(st)); if (rc < 0) return rc;
  rc = launch_stem_gram(dt, x, gram, gram_floats, R, N, Sz, H1, H1, stream_of(st));
  if (rc < 0) return rc;
  const int np = launch_stem_bwd_dg(dy1, dys, pk1, pks, y0, x, bn_scale, bn_shift, part, part_floats, N, Sz, H1, H1, stream_of(st));
  if (np < 0) return np;
  return launch_stem_bwd_finalize(part, np, R, w, nullptr, (double)N * H1 * H1, gamma, save_mean, save_istd, dgamma, dbeta, dw, stream_of(st));
}
int mmvae_tail_join_fwd(int dt, const void* y2, const float* s2, const float* b2, const void* ys, const float* ss, const float* bs,
                        const float* w, const float* bias, float* r_raw, float* stats, int N, int H, int W, void* st) {
  return launch_tail_join_fwd(dt, BnSide{y2, {s2, b2}}, BnSide{ys, {ss, bs}}, w, bias, r_raw, stats, N, H, W, stream_of(st));
}
int mmvae_tail_join_fwd_stream(int dt, const void* y2, const float* s2, const float* b2, const void* ys, const float* ss, const float* bs,
                               const float* w, const float* bias, float* r_raw, float* stats, int N, int H, int W, void* st) {
  return launch_tail_fwd_stream(dt, BnSide{y2, {s2, b2}}, BnSide{ys, {ss, bs}}, w, bias, r_raw, stats, N, H, W, stream_of(st));
}
int mmvae_tail_join_bwd_reduce(int dt, const float* d_raw, const float* w, int oc, const void* y2, const float* s2, const float* b2,
                               const void* ys, const float* ss, const float* bs, float* partials, float* wpartials, int N, int H, int W,
                               void* st) {
  return launch_tail_join_bwd_reduce(dt, d_raw, w, BnSide{y2, {s2, b2}}, BnSide{ys, {ss, bs}}, partials, oc, N, H, W, stream_of(st), wpartials);
}
int mmvae_tail_join_bwd_apply(int dt, const float* d_raw, const float* w, int oc, const void* y2, const float* s2, const float* b2,
                              const void* ys, const float* ss, const float* bs, const float* A2, const float* B2, const float* C2,
                              const float* As, const float* Bs, const float* Cs, void* dy2, void* dys, int N, int H, int W, void* st) {
  return launch_tail_join_bwd_apply(dt, d_raw, w, BnSide{y2, {s2, b2}, {A2, B2, C2}}, BnSide{ys, {ss, bs}, {As, Bs, Cs}}, dy2, dys, oc, N, H, W, stream_of(st));
}
int mmvae_upblock_bwd_fused(const float* d_raw, const float* tw, const void* y2, const float* s2, const float* b2, const void* ys, const float* ss,
                            const float* bs, const float* A2, const float* B2, const float* C2, const float* As, const float* Bs, const float* Cs,
                            const void* y1, const float* s1, const float* b1, const float* w2, float* dw2, void* da1, float* bn1_sums,
                            const void* xin, const float* sx, const float* bx, const float* wu, float* dwu, void* gin, int N, void* scratch, void* st) {
  if (!scratch || !d_raw || !tw || !y2 || !ys || !y1 || !xin || !w2 || !wu || !dw2 || !dwu || !da1 || !gin || !bn1_sums || N < 1 || ((sx != nullptr) != (bx != nullptr))) {
    set_error("upblock_bwd_fused: bad argument"); return MMVAE_ERR_ARG;
  }
  char* sc = static_cast<char*>(scratch);
  const ConvGeom g = geom_for(1, 16, 16, 4, 2, 1);
  int rc = op_pack_down(DT_BF16, g, w2, sc, stream_of(st)); if (rc < 0) return rc;
  rc = op_pack_down(DT_BF16, g, wu, sc + 8192, stream_of(st)); if (rc < 0) return rc;
  float* parts = reinterpret_cast<float*>(sc + 16384);
  JoinBwdLaunch L;
  L.d_raw = d_raw; L.w_tail = tw; L.y2 = BnSide{y2, {s2, b2}, {A2, B2, C2}}; L.ys = BnSide{ys, {ss, bs}, {As, Bs, Cs}};
  L.y1 = BnSide{y1, {s1, b1}}; L.wd2 = sc; L.da1 = da1; L.part2 = parts; L.bn_part = parts + 2L * 1024 * 4096;
  L.xin = BnSide{xin, {sx, bx}}; L.wds = sc + 8192; L.gin = gin; L.parts = parts + 1024L * 4096;
  L.N = N;
  const int nb = launch_join_bwd_stream(L, stream_of(st));
  if (nb < 0) return nb;
  rc = launch_wgrad_reduce(reduce_args(L.part2, nb, dw2, 16, 16, 16), stream_of(st)); if (rc < 0) return rc;
  rc = launch_wgrad_reduce(reduce_args(L.parts, nb, dwu, 16, 16, 16), stream_of(st)); if (rc < 0) return rc;
  return launch_partial_rowsum(L.bn_part, nb, 32, bn1_sums, stream_of(st));
}
int mmvae_upblock_tail_fwd(const void* y1, const float* s1, const float* b1, const float* w2, const void* xin, const float* sx, const float* bx,
                           const float* wu, const float* s2, const float* b2, const float* ss, const float* bs, const float* tw, const float* bias,
                           float* r_raw, float* stats, int N, void* scratch, void* st) {
  if (!scratch || !y1 || !s1 || !b1 || !w2 || !xin || !wu || !s2 || !b2 || !ss || !bs || !tw || !r_raw || N < 1 || ((sx != nullptr) != (bx != nullptr))) {
    set_error("upblock_tail_fwd: bad argument"); return MMVAE_ERR_ARG;
  }
  char* sc = static_cast<char*>(scratch);
  const ConvGeom g = geom_for(1, 16, 16, 4, 2, 1);
  int rc = op_pack_up(DT_BF16, g, w2, sc, stream_of(st)); if (rc < 0) return rc;
  rc = op_pack_up(DT_BF16, g, wu, sc + 8192, stream_of(st)); if (rc < 0) return rc;
  return launch_up5_tail_fwd(BnSide{y1, {s1, b1}}, sc, BnSide{xin, {sx, bx}}, sc + 8192, Affine{s2, b2}, Affine{ss, bs}, tw, bias, r_raw, stats, N, stream_of(st));
}
int mmvae_upblock_tail_fwd_store(const void* y1, const float* s1, const float* b1, const float* w2, const void* xin, const float* sx, const float* bx,
                                 const float* wu, const float* s2, const float* b2, const float* ss, const float* bs, const float* tw,
                                 const float* bias, float* r_raw, float* stats, void* y2, void* ys, int N, void* scratch, void* st) {
  if (!scratch || !y1 || !s1 || !b1 || !w2 || !xin || !wu || !s2 || !b2 || !ss || !bs || !tw || !r_raw || !y2 || !ys || N < 1 ||
      ((sx != nullptr) != (bx != nullptr))) {
    set_error("upblock_tail_fwd_store: bad argument"); return MMVAE_ERR_ARG;
  }
  char* sc = static_cast<char*>(scratch);
  const ConvGeom g = geom_for(1, 16, 16, 4, 2, 1);
  int rc = op_pack_up(DT_BF16, g, w2, sc, stream_of(st)); if (rc < 0) return rc;
  rc = op_pack_up(DT_BF16, g, wu, sc + 8192, stream_of(st)); if (rc < 0) return rc;
  return launch_up5_tail_fwd(BnSide{y1, {s1, b1}}, sc, BnSide{xin, {sx, bx}}, sc + 8192, Affine{s2, b2}, Affine{ss, bs}, tw, bias, r_raw, stats, N, stream_of(st), y2, ys);
}
int mmvae_convT4_stats(int dt, const void* x, const float* w, const float* ps, const float* pb, float* stats, int N, int e4m3_out, void* scratch,
                       void* st) {
  if (!scratch || !x || !w || !stats || N < 1 || ((ps != nullptr) != (pb != nullptr))) { set_error("convT4_stats: bad argument"); return MMVAE_ERR_ARG; }
  if (dt != DT_BF16) { set_error("convT4_stats: bf16 only"); return MMVAE_ERR_UNSUPPORTED; }
  if (e4m3_out) { set_error("convT4_stats: the e4m3 storage mode has no statistics-only form"); return MMVAE_ERR_UNSUPPORTED; }
  int rc = op_pack_up(dt, geom_for(1, 16, 16, 4, 2, 1), w, scratch, stream_of(st)); if (rc < 0) return rc;
  return launch_convT4_stream(dt, MapIn(BnSide{x, {ps, pb}}, 32, 32), scratch, MapOut(nullptr, 64, 64, stats), N, stream_of(st));
}
int mmvae_conv1x1_bwd_fused(const void* da1, const void* y1, const float* s1, const float* b1, const float* A1, const float* B1, const float* C1,
                            const void* xin, const float* sx, const float* bx, const float* w1, float* dw1, void* gin, int64_t rows, void* scratch,
                            void* st) {
  if (!scratch || !da1 || !y1 || !s1 || !b1 || !A1 || !B1 || !C1 || !xin || !w1 || !dw1 || !gin || rows < 1 || ((sx != nullptr) != (bx != nullptr))) {
    set_error("conv1x1_bwd_fused: bad argument"); return MMVAE_ERR_ARG;
  }
  char* sc = static_cast<char*>(scratch);
  const ConvGeom g = geom_for(0, 16, 16, 1, 1, 0);
  int rc = op_pack_up(DT_BF16, g, w1, sc, stream_of(st)); if (rc < 0) return rc;
  Conv1BwdLaunch C;
  C.da1 = da1; C.y1 = BnSide{y1, {s1, b1}, {A1, B1, C1}}; C.xin = BnSide{xin, {sx, bx}}; C.w1u = sc; C.gin = gin;
  C.part = reinterpret_cast<float*>(sc + 4096); C.nrows = (long)rows;
  const int nb = launch_conv1_bwd_stream(C, stream_of(st));
  if (nb < 0) return nb;
  return launch_wgrad_reduce(reduce_args(C.part, nb, dw1, 16, 16, 1), stream_of(st));
}
int mmvae_join_conv1x1_fwd(const void* y2, const float* s2, const float* b2, const void* ys, const float* ss, const float* bs, const float* w1, int C,
                           void* out, void* y1, float* stats, int64_t npix, void* scratch, void* st) {
  if (!y2 || !s2 || !b2 || !ys || !ss || !bs || !w1 || !out || !y1 || !scratch) { set_error("join_conv1x1_fwd: bad argument"); return MMVAE_ERR_ARG; }
  if (!join_conv1_fwd_ok(DT_BF16, C, 16, (long)npix)) { set_error("join_conv1x1_fwd: C=%d npix=%ld unsupported (16 / 32 channels, whole 32-pixel steps)", C, (long)npix); return MMVAE_ERR_UNSUPPORTED; }
  const ConvGeom g = geom_for(0, C, 16, 1, 1, 0);
  const int rc = op_pack_down(DT_BF16, g, w1, scratch, stream_of(st)); if (rc < 0) return rc;
  return launch_join_conv1_fwd(BnSide{y2, {s2, b2}}, BnSide{ys, {ss, bs}}, scratch, out, y1, stats, C, (long)npix, stream_of(st));
}
int mmvae_convert(int di, int dout, const void* in, void* out, int64_t n, void* st) { return launch_convert(di, dout, in, out, (long)n, stream_of(st)); }

}  // extern "C"

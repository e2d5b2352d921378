// C-ABI glue for the Extract stage: weight preparation (fp32 checkpoint -> e16 device layout,
// conv+linear folding, QKV concatenation, constant query precompute) and the launch sequence of
// _Spec2MIDI.forward / AMTAPC_Extractor._transcript (etude/data/extractor.py:53-56,199-253).
#include <string>
#include <vector>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../../include/etude_hip_debug.h"
#include "ext_kernels.h"
#include "ext_fp32.h"

thread_local std::string g_etd_err;
extern "C" const char* etd_last_error(void) { return g_etd_err.c_str(); }
extern "C" int etd_version(void) { return ETD_ABI_VERSION; }

namespace {

// fp32 -> the extractor's 16-bit operand type (ext_kernels.h: IEEE half by default, bf16 under -DETD_EXT_BF16), round-to-nearest-even, NaN kept; and back
#if ETD_EXT_IS_F16
inline uint16_t f2bf(float f) { return f32_to_f16_bits(f); }
inline float e2f(uint16_t q) { _Float16 h; memcpy(&h, &q, 2); return (float)h; }
#else
inline uint16_t f2bf(float f) { return f32_to_bf16_bits(f); }
inline float e2f(uint16_t q) { const uint32_t u = (uint32_t)q << 16; float w; memcpy(&w, &u, 4); return w; }
#endif

struct LinW { e16* W = nullptr; float* b = nullptr; };
// p*: the same Linear weights as 256 x 256 blocks in k_proj256's fragment-ordered stream (ext_fused.hip); ffn: k_ffn_fused's stream
struct EncLayerW { LinW qkv, o, f1, f2; float *g = nullptr, *be = nullptr; e16 *ffn = nullptr, *pq = nullptr, *pk = nullptr, *pv = nullptr, *po = nullptr;
                   e16* lw = nullptr; /* k_enc_layer's whole-layer stream (32 x 32 KiB) */ };
struct DecLayerW { LinW qkv_s, o_s, q_c, kv_c, o_c, f1, f2; float *g = nullptr, *be = nullptr; bool has_self = false; e16* ffn = nullptr;
                   e16 *pq = nullptr, *pk = nullptr, *pv = nullptr, *po = nullptr, *pqc = nullptr, *pkc = nullptr, *pvc = nullptr, *poc = nullptr; };

}  // namespace

struct etd_ext {
  etd_ext_cfg cfg;
  DevPool pool;                // everything the extractor allocates; freed in destroy
  int nf, nn, margin, wb, fc;
  // weights
  e16* Wf = nullptr; float* bfold = nullptr; e16* pos_freq_enc = nullptr;
  EncLayerW enc[3];
  DecLayerW dec[3];
  e16* q0 = nullptr;          // fc_q(pos_embedding_freq) of layer zero, [nn][256]
  e16* trg0 = nullptr;        // decoder.pos_embedding_freq [nn][256]
  float* pos_time = nullptr;   // [nf][256] fp32
  EncLayerW tim[3];
  LinW head_time, head_freq;   // [160][256]
  float* bkv_all = nullptr;    // biases of the 3 cross-attention K/V projections, [3][k 256 | v 256]
  // workspaces (e16 unless noted)
  size_t MT = 0, MQ = 0;       // token capacities
  e16 *X = nullptr, *X1 = nullptr, *QK = nullptr, *VT = nullptr, *AO = nullptr;
  e16 *Tq = nullptr, *T1 = nullptr, *QKd = nullptr, *VTd = nullptr, *AOd = nullptr, *Qd = nullptr, *Tfreq = nullptr;
  e16* TI = nullptr;          // time-decoder input [wb*nn*nf][256]
  e16 *KVimg = nullptr, *KVcimg = nullptr;   // K / V MFMA-fragment images for k_attn_frag: self-attention [MT * 512], cross-attention [3][MTe * 512]
  size_t MTe = 0;              // encoder chunk token capacity (wb*fc*256)
  float* dbg_vel = nullptr;
  void* tap[16] = {nullptr};   // test hook: device destinations for intermediate activations (first chunk only)
  Ext32* f32 = nullptr;        // fp32 parity mode (cfg.precision == 1): its own weights and workspaces, none of the above
};

namespace {

int up_bf16(DevPool& pool, e16** dst, const float* src, size_t n) {
  std::vector<uint16_t> h(n);
  for (size_t i = 0; i < n; ++i) h[i] = f2bf(src[i]);
  return pool.upload(dst, h.data(), n);
}
int load_lin(DevPool& pool, const WeightTable& L, const std::string& pfx, int out_f, int in_f, LinW* w) {
  const float* W = L.get(pfx + ".weight", (int64_t)out_f * in_f);
  const float* b = L.get(pfx + ".bias", out_f);
  if (!W || !b) return ETD_EINVAL;
  ETD_TRY(up_bf16(pool, &w->W, W, (size_t)out_f * in_f));
  ETD_TRY(pool.upload(&w->b, b, out_f));
  return ETD_OK;
}
// concatenate several [256][256] linears along the output dim
int load_cat(DevPool& pool, const WeightTable& L, const std::vector<std::string>& pfx, LinW* w, std::vector<float>* keepB = nullptr) {
  std::vector<float> W, b;
  for (auto& p : pfx) {
    const float* Wi = L.get(p + ".weight", 256 * 256);
    const float* bi = L.get(p + ".bias", 256);
    if (!Wi || !bi) return ETD_EINVAL;
    W.insert(W.end(), Wi, Wi + 256 * 256);
    b.insert(b.end(), bi, bi + 256);
  }
  ETD_TRY(up_bf16(pool, &w->W, W.data(), W.size()));
  ETD_TRY(pool.upload(&w->b, b.data(), b.size()));
  if (keepB) *keepB = b;
  return ETD_OK;
}
int load_ln(DevPool& pool, const WeightTable& L, const std::string& pfx, float** g, float** b) {
  const float* gw = L.get(pfx + ".weight", 256);
  const float* bw = L.get(pfx + ".bias", 256);
  if (!gw || !bw) return ETD_EINVAL;
  ETD_TRY(pool.upload(g, gw, 256));
  ETD_TRY(pool.upload(b, bw, 256));
  return ETD_OK;
}
// fc_1 / fc_2 of a position-wise feed-forward block in the fused kernel's fragment-ordered stream
int load_ffn_stream(DevPool& pool, const WeightTable& L, const std::string& p, e16** dst) {
  const float* W1 = L.get(p + ".fc_1.weight", 512 * 256);
  const float* W2 = L.get(p + ".fc_2.weight", 256 * 512);
  if (!W1 || !W2) return ETD_EINVAL;
  std::vector<uint16_t> h((size_t)16 * 32 * 64 * 8);
  pack_ffn_weights(W1, W2, h.data(), f2bf);
  return pool.upload(dst, h.data(), h.size());
}
// one [256][256] Linear as a k_proj256 block (rows permuted for row-major / LayerNorm blocks, natural for V^T blocks)
int load_proj_block(DevPool& pool, const WeightTable& L, const std::string& name, bool permute_rows, e16** dst) {
  const float* W = L.get(name + ".weight", 256 * 256);
  if (!W) return ETD_EINVAL;
  std::vector<uint16_t> h((size_t)256 * 256);
  pack_proj_weights(W, permute_rows, h.data(), f2bf);
  return pool.upload(dst, h.data(), h.size());
}
int load_enc_layer(DevPool& pool, const WeightTable& L, const std::string& p, EncLayerW* w) {
  ETD_TRY(load_ffn_stream(pool, L, p + ".positionwise_feedforward", &w->ffn));
  ETD_TRY(load_proj_block(pool, L, p + ".self_attention.fc_q", true, &w->pq));
  ETD_TRY(load_proj_block(pool, L, p + ".self_attention.fc_k", true, &w->pk));
  ETD_TRY(load_proj_block(pool, L, p + ".self_attention.fc_v", false, &w->pv));
  ETD_TRY(load_proj_block(pool, L, p + ".self_attention.fc_o", true, &w->po));
  {
    const float* Wq = L.get(p + ".self_attention.fc_q.weight", 65536); const float* Wk = L.get(p + ".self_attention.fc_k.weight", 65536);
    const float* Wv = L.get(p + ".self_attention.fc_v.weight", 65536); const float* Wo = L.get(p + ".self_attention.fc_o.weight", 65536);
    const float* W1 = L.get(p + ".positionwise_feedforward.fc_1.weight", 512 * 256); const float* W2 = L.get(p + ".positionwise_feedforward.fc_2.weight", 256 * 512);
    if (!Wq || !Wk || !Wv || !Wo || !W1 || !W2) return ETD_EINVAL;
    std::vector<uint16_t> h((size_t)32 * 16384);
    pack_enc_layer_weights(Wq, Wk, Wv, Wo, W1, W2, h.data(), f2bf);
    ETD_TRY(pool.upload(&w->lw, h.data(), h.size()));
  }
  ETD_TRY(load_cat(pool, L, {p + ".self_attention.fc_q", p + ".self_attention.fc_k", p + ".self_attention.fc_v"}, &w->qkv));
  ETD_TRY(load_lin(pool, L, p + ".self_attention.fc_o", 256, 256, &w->o));
  ETD_TRY(load_lin(pool, L, p + ".positionwise_feedforward.fc_1", 512, 256, &w->f1));
  ETD_TRY(load_lin(pool, L, p + ".positionwise_feedforward.fc_2", 256, 512, &w->f2));
  ETD_TRY(load_ln(pool, L, p + ".layer_norm", &w->g, &w->be));
  return ETD_OK;
}
int load_heads(DevPool& pool, const WeightTable& L, const std::string& sfx, LinW* w) {
  std::vector<float> W(160 * 256, 0.f), b(160, 0.f);
  const float* vw = L.get("decoder.fc_velocity_" + sfx + ".weight", 128 * 256);
  const float* vb = L.get("decoder.fc_velocity_" + sfx + ".bias", 128);
  if (!vw || !vb) return ETD_EINVAL;
  memcpy(W.data(), vw, 128 * 256 * 4);
  memcpy(b.data(), vb, 128 * 4);
  const char* nm[3] = {"onset", "offset", "mpe"};
  for (int i = 0; i < 3; ++i) {
    const float* hw = L.get(std::string("decoder.fc_") + nm[i] + "_" + sfx + ".weight", 256);
    const float* hb = L.get(std::string("decoder.fc_") + nm[i] + "_" + sfx + ".bias", 1);
    if (!hw || !hb) return ETD_EINVAL;
    memcpy(W.data() + (128 + i) * 256, hw, 256 * 4);
    b[128 + i] = hb[0];
  }
  ETD_TRY(up_bf16(pool, &w->W, W.data(), W.size()));
  ETD_TRY(pool.upload(&w->b, b.data(), b.size()));
  return ETD_OK;
}

}  // namespace

extern "C" int etd_extractor_operand_type(void) { return ETD_EXT_IS_F16; }

extern "C" int etd_extractor_create(const etd_ext_cfg* cfg, const char* const* names, const float* const* host_ptrs,
                                    const int64_t* numels, int n, etd_ext** out) {
  if (!cfg || !names || !host_ptrs || !numels || !out) ETD_FAIL(ETD_EINVAL, "extractor_create: null argument");
  if (cfg->struct_bytes != (int)sizeof(etd_ext_cfg)) ETD_FAIL(ETD_EINVAL, "extractor_create: etd_ext_cfg of %d bytes, this library (ABI %d) expects %d -- caller built against another etude_hip.h", cfg->struct_bytes, ETD_ABI_VERSION, (int)sizeof(etd_ext_cfg));
  const etd_ext_cfg& c = *cfg;
  // The 16-bit serving kernels are specialised for the reference's default architecture (schema.py:103-112); the exact-parity engine (precision 1, csrc/ext_fp32.hip)
  // takes every architecture with head_dim 64 and checks its own limits.
  const bool dflt_arch = c.hid_dim == 256 && c.n_heads == 4 && c.pf_dim == 512 && c.n_bin == 256 && c.n_margin == 32 && c.cnn_channel == 4 && c.cnn_kernel == 5 &&
                         c.n_layers_enc == 3 && c.n_layers_dec == 3 && c.n_velocity == 128;
  if (c.precision == 0 && !dflt_arch)
    ETD_FAIL(ETD_EINVAL, "extractor_create: unsupported architecture for the 16-bit serving mode (its kernels are built for hid 256 / 4 heads / pf 512 / 256 bins / margin 32 / cnn 4x5 / 3+3 layers / 128 velocities); "
                         "precision = 1 selects the general engine, which takes any architecture with head_dim 64");
  if (c.precision == 0 && (c.n_frame < 32 || c.n_frame % 32 || c.n_note < 4 || c.n_note % 4 || c.n_note > 128))
    ETD_FAIL(ETD_EINVAL, "extractor_create: the 16-bit serving mode needs n_frame %% 32 == 0, n_note %% 4 == 0 and <= 128");
  if (c.n_frame < 1 || c.n_note < 1 || c.max_windows < 1) ETD_FAIL(ETD_EINVAL, "extractor_create: need n_frame >= 1, n_note >= 1, max_windows >= 1");
  if (c.precision != 0 && c.precision != 1) ETD_FAIL(ETD_EINVAL, "extractor_create: precision must be 0 (e16) or 1 (fp32 parity mode)");
  etd_ext* e = new etd_ext();
  e->cfg = c; e->nf = c.n_frame; e->nn = c.n_note; e->margin = c.n_margin; e->wb = c.max_windows;
  e->fc = c.chunk_frames > 0 ? c.chunk_frames : c.n_frame;   // measured: whole-window launches beat MALL-sized chunks (2.9 vs 4.4 ms/window)
  if (e->fc > e->nf) e->fc = e->nf;
  if (e->fc < 1) e->fc = e->nf;
  const WeightTable L(names, host_ptrs, numels, n);
  DevPool& P = e->pool;
  auto fail = [&](int rc) { e->pool.free_all(); ext32_destroy(e->f32); delete e; return rc; };
  auto sync = [] { if (hipDeviceSynchronize() == hipSuccess) return ETD_OK; g_etd_err = "extractor_create: device synchronisation failed"; return ETD_EHIP; };
  if (c.precision == 1) {
    ETD_TRY_OR(fail, ext32_create(c, L, &e->f32));
    ETD_TRY_OR(fail, sync());
    *out = e;
    return ETD_OK;
  }

  // ---- front end: fold Conv2d(1,4,(1,5)) and Linear(244,256) into one [256][65] map (amt_apc.py:79-99)
  {
    const float* cw = L.get("encoder.conv.weight", 4 * 5);
    const float* cb = L.get("encoder.conv.bias", 4);
    const float* tw = L.get("encoder.tok_embedding_freq.weight", 256 * 244);
    const float* tb = L.get("encoder.tok_embedding_freq.bias", 256);
    const float* pe = L.get("encoder.pos_embedding_freq.weight", 256 * 256);
    if (!cw || !cb || !tw || !tb || !pe) return fail(ETD_EINVAL);
    const float center = -8.0f;
    std::vector<float> Wf(256 * 80, 0.f), bf(256);
    for (int o = 0; o < 256; ++o) {
      double fold[65] = {0};
      double bacc = tb[o];
      for (int ch = 0; ch < 4; ++ch)
        for (int p = 0; p < 61; ++p) {
          const double w = tw[o * 244 + ch * 61 + p];
          bacc += w * cb[ch];
          for (int k = 0; k < 5; ++k) fold[p + k] += w * cw[ch * 5 + k];
        }
      double wsum = 0;
      for (int t = 0; t < 65; ++t) {
        Wf[o * 80 + t] = (float)fold[t];
        wsum += e2f(f2bf((float)fold[t]));                                // the kernel multiplies by the e16-rounded weight
      }
      bf[o] = (float)(bacc + (double)center * wsum);  // x = (x - center) + center
    }
#if ETD_EXT_IS_F16
    {
      // IEEE-half operands end at 65 504 (bf16 did not): the only 16-bit tensor of this path that no LayerNorm bounds is the first encoder layer's input,
      // x = 16 (Wf . window + b) + pos, for log-mel features in [-F, F] (F = max(|min_value|, 32): log(mel + 1e-8) >= -18.4 and full-scale audio stays below 15;
      // the HFT_Transformer wrapper pads with -80).  Its worst case over such inputs, from the folded weights; a checkpoint that could leave the range is refused.
      const float F = fmaxf(fabsf(c.min_value), 32.f);
      float pmax = 0.f, xb = 0.f;
      for (int i = 0; i < 256 * 256; ++i) pmax = fmaxf(pmax, fabsf(pe[i]));
      for (int o = 0; o < 256; ++o) {
        double l1 = 0;
        for (int t = 0; t < 65; ++t) l1 += fabs((double)Wf[o * 80 + t]);
        xb = fmaxf(xb, (float)(16.0 * (l1 * (F + 8.0) + fabs((double)bf[o]))));      // (the kernel feeds x - center, center = -8)
      }
      if (!(xb + pmax < 65504.f)) {
        g_etd_err = "extractor_create: the first encoder layer's input can reach " + std::to_string(xb + pmax) + " for log-mel features in [-" + std::to_string((int)F) + ", " + std::to_string((int)F) +
                    "], beyond the IEEE-half range of the 16-bit mode; use precision \"fp32\" (etd_ext_cfg.precision 1) or a -DETD_EXT_BF16 build";
        return fail(ETD_EINVAL);
      }
    }
#endif
    ETD_TRY_OR(fail, up_bf16(P, &e->Wf, Wf.data(), Wf.size()));
    ETD_TRY_OR(fail, P.upload(&e->bfold, bf.data(), 256));
    ETD_TRY_OR(fail, up_bf16(P, &e->pos_freq_enc, pe, 256 * 256));
  }
  for (int i = 0; i < 3; ++i) ETD_TRY_OR(fail, load_enc_layer(P, L, "encoder.layers_freq." + std::to_string(i), &e->enc[i]));
  for (int i = 0; i < 3; ++i) ETD_TRY_OR(fail, load_enc_layer(P, L, "decoder.layers_time." + std::to_string(i), &e->tim[i]));
  // ---- frequency decoder
  std::vector<float> kvB;
  for (int i = 0; i < 3; ++i) {
    const std::string p = i == 0 ? std::string("decoder.layer_zero_freq") : "decoder.layers_freq." + std::to_string(i - 1);
    DecLayerW& w = e->dec[i];
    w.has_self = i > 0;
    if (w.has_self) {
      ETD_TRY_OR(fail, load_cat(P, L, {p + ".self_attention.fc_q", p + ".self_attention.fc_k", p + ".self_attention.fc_v"}, &w.qkv_s));
      ETD_TRY_OR(fail, load_lin(P, L, p + ".self_attention.fc_o", 256, 256, &w.o_s));
      ETD_TRY_OR(fail, load_proj_block(P, L, p + ".self_attention.fc_q", true, &w.pq));
      ETD_TRY_OR(fail, load_proj_block(P, L, p + ".self_attention.fc_k", true, &w.pk));
      ETD_TRY_OR(fail, load_proj_block(P, L, p + ".self_attention.fc_v", false, &w.pv));
      ETD_TRY_OR(fail, load_proj_block(P, L, p + ".self_attention.fc_o", true, &w.po));
    }
    ETD_TRY_OR(fail, load_proj_block(P, L, p + ".encoder_attention.fc_q", true, &w.pqc));
    ETD_TRY_OR(fail, load_proj_block(P, L, p + ".encoder_attention.fc_k", true, &w.pkc));
    ETD_TRY_OR(fail, load_proj_block(P, L, p + ".encoder_attention.fc_v", false, &w.pvc));
    ETD_TRY_OR(fail, load_proj_block(P, L, p + ".encoder_attention.fc_o", true, &w.poc));
    ETD_TRY_OR(fail, load_lin(P, L, p + ".encoder_attention.fc_q", 256, 256, &w.q_c));
    std::vector<float> b1;
    ETD_TRY_OR(fail, load_cat(P, L, {p + ".encoder_attention.fc_k", p + ".encoder_attention.fc_v"}, &w.kv_c, &b1));
    kvB.insert(kvB.end(), b1.begin(), b1.end());
    ETD_TRY_OR(fail, load_lin(P, L, p + ".encoder_attention.fc_o", 256, 256, &w.o_c));
    ETD_TRY_OR(fail, load_lin(P, L, p + ".positionwise_feedforward.fc_1", 512, 256, &w.f1));
    ETD_TRY_OR(fail, load_lin(P, L, p + ".positionwise_feedforward.fc_2", 256, 512, &w.f2));
    ETD_TRY_OR(fail, load_ffn_stream(P, L, p + ".positionwise_feedforward", &w.ffn));
    ETD_TRY_OR(fail, load_ln(P, L, p + ".layer_norm", &w.g, &w.be));
  }
  ETD_TRY_OR(fail, P.upload(&e->bkv_all, kvB.data(), kvB.size()));
  {
    const int nn = e->nn;
    const float* pe = L.get("decoder.pos_embedding_freq.weight", (int64_t)nn * 256);
    const float* qw = L.get("decoder.layer_zero_freq.encoder_attention.fc_q.weight", 256 * 256);
    const float* qb = L.get("decoder.layer_zero_freq.encoder_attention.fc_q.bias", 256);
    const float* pt = L.get("decoder.pos_embedding_time.weight", (int64_t)e->nf * 256);
    if (!pe || !qw || !qb || !pt) return fail(ETD_EINVAL);
    // layer-zero queries are input independent: fc_q(pos_embedding_freq) (amt_apc.py:168-175,342)
    std::vector<float> q0((size_t)nn * 256);
    for (int r = 0; r < nn; ++r)
      for (int o = 0; o < 256; ++o) {
        double s = qb[o];
        for (int k = 0; k < 256; ++k) s += (double)pe[r * 256 + k] * qw[o * 256 + k];
        q0[(size_t)r * 256 + o] = (float)s;
      }
    ETD_TRY_OR(fail, up_bf16(P, &e->q0, q0.data(), q0.size()));
    ETD_TRY_OR(fail, up_bf16(P, &e->trg0, pe, (size_t)nn * 256));
    ETD_TRY_OR(fail, P.upload(&e->pos_time, pt, (size_t)e->nf * 256));
  }
  ETD_TRY_OR(fail, load_heads(P, L, "time", &e->head_time));
  ETD_TRY_OR(fail, load_heads(P, L, "freq", &e->head_freq));

  // ---- workspaces
  const size_t MTe = (size_t)e->wb * e->fc * 256;           // encoder tokens per chunk
  const size_t MTt = (size_t)e->wb * e->nn * e->nf;         // time-decoder tokens per window batch
  const size_t MT = MTe > MTt ? MTe : MTt;
  const size_t MQ = (size_t)e->wb * e->fc * e->nn;          // freq-decoder query tokens per chunk
  e->MT = MT; e->MQ = MQ; e->MTe = MTe;
  ETD_TRY_OR(fail, P.alloc(&e->X, MT * 256));
  ETD_TRY_OR(fail, P.alloc(&e->X1, MT * 256));
  ETD_TRY_OR(fail, P.alloc(&e->QK, MT * 512));
  ETD_TRY_OR(fail, P.alloc(&e->VT, MT * 256, true));
  ETD_TRY_OR(fail, P.alloc(&e->AO, MT * 256));
  ETD_TRY_OR(fail, P.alloc(&e->Tq, MQ * 256));
  ETD_TRY_OR(fail, P.alloc(&e->T1, MQ * 256));
  ETD_TRY_OR(fail, P.alloc(&e->Tfreq, MQ * 256));
  ETD_TRY_OR(fail, P.alloc(&e->QKd, MQ * 512));
  ETD_TRY_OR(fail, P.alloc(&e->VTd, (size_t)e->wb * e->fc * 4 * 64 * 128, true));   // S = nn <= 128 padded to 128; pad stays 0
  ETD_TRY_OR(fail, P.alloc(&e->AOd, MQ * 256));
  ETD_TRY_OR(fail, P.alloc(&e->Qd, MQ * 256));
  ETD_TRY_OR(fail, P.alloc(&e->TI, MTt * 256));
  ETD_TRY_OR(fail, P.alloc(&e->KVimg, MT * 512));
  ETD_TRY_OR(fail, P.alloc(&e->KVcimg, 3 * MTe * 512));
  ETD_TRY_OR(fail, sync());
  *out = e;
  return ETD_OK;
}

extern "C" void etd_extractor_destroy(etd_ext* e) {
  if (!e) return;
  (void)hipDeviceSynchronize();   // kernels of this handle may still be in flight
  e->pool.free_all();
  ext32_destroy(e->f32);
  delete e;
}

extern "C" int etd_extractor_debug_vel_logits(etd_ext* e, float* p) { if (!e) ETD_FAIL(ETD_EINVAL, "null"); e->dbg_vel = p; return ETD_OK; }

extern "C" int etd_extractor_debug_tap(etd_ext* e, int stage, void* dst_dev) {
  if (!e || stage < 0 || stage >= 16) ETD_FAIL(ETD_EINVAL, "debug_tap: bad stage");
  e->tap[stage] = dst_dev;
  return ETD_OK;
}

extern "C" double etd_extractor_window_flops(const etd_ext* e) {
  // lin(t,i,o)=2tio; attn(N,q,k)=4*N*q*k*hid (n_heads x 64)
  const etd_ext_cfg& c = e->cfg;
  const double nf = e->nf, nb = c.n_bin, nn = e->nn, H = c.hid_dim, PF = c.pf_dim, LE = c.n_layers_enc, LD = c.n_layers_dec;
  const double P = 2 * c.n_margin + 1 - (c.cnn_kernel - 1), nhead = c.n_velocity + 3;
  auto lin = [](double t, double i, double o) { return 2 * t * i * o; };
  auto attn = [H](double N, double q, double k) { return 4 * N * q * k * H; };
  const double te = nf * nb, tq = nf * nn;
  double enc_layer = 4 * lin(te, H, H) + attn(nf, nb, nb) + lin(te, H, PF) + lin(te, PF, H);
  double conv = 2 * te * c.cnn_channel * P * c.cnn_kernel, embed = lin(te, c.cnn_channel * P, H);
  double d0 = lin(tq, H, H) + 2 * lin(te, H, H) + attn(nf, nn, nb) + lin(tq, H, H) + lin(tq, H, PF) + lin(tq, PF, H);
  double dn = d0 + 4 * lin(tq, H, H) + attn(nf, nn, nn);
  double heads = lin(tq, H, nhead);
  double time_layer = 4 * lin(tq, H, H) + attn(nn, nf, nf) + lin(tq, H, PF) + lin(tq, PF, H);
  return conv + embed + LE * enc_layer + d0 + (LD - 1) * dn + heads + LD * time_layer + heads;
}

namespace {

const float kScaleLog2e = 0.125f * 1.4426950408889634f;
ProjBlock pblock(const e16* Wf, const float* bias, int kind, e16* dst, int ldd, int relu = 0) {
  ProjBlock b = {}; b.Wf = Wf; b.bias = bias; b.kind = kind; b.relu = relu; b.dst = dst; b.ldd = ldd; return b;
}
// Q | K row-major into QK[tok][512], V transposed into VT: ONE launch, the token tile is read once
int proj_qkv(const e16* X, int M, const e16* pq, const e16* pk, const e16* pv, const float* bias768, e16* QK, e16* VT, int S, int Spad, hipStream_t st) {
  ProjArgs a = {};
  a.X = X; a.ldx = 256; a.M = M; a.nblk = 3; a.S = S; a.Spad = Spad;
  a.blk[0] = pblock(pq, bias768, PROJ_ROW, QK, 512);
  a.blk[1] = pblock(pk, bias768 + 256, PROJ_ROW, QK + 256, 512);
  a.blk[2] = pblock(pv, bias768 + 512, PROJ_VT, VT, 0);
  return launch_proj256(a, st);
}
// Y = LN(R + X Wo^T + b) * gamma + beta
int proj_ln(const e16* X, int M, const e16* po, const float* bias, const e16* R, int r_mod, const float* g, const float* be, e16* Y, hipStream_t st) {
  ProjArgs a = {};
  a.X = X; a.ldx = 256; a.M = M; a.nblk = 1; a.R = R; a.r_mod = r_mod; a.gamma = g; a.beta = be;
  a.blk[0] = pblock(po, bias, PROJ_LN, Y, 256);
  return launch_proj256(a, st);
}

int enc_like_layer(etd_ext* e, const EncLayerW& w, e16* X, e16* X1, int M, int n_seq, int S, hipStream_t st,
                   e16* Yfinal /* where the 2nd LN writes (X to run in place) */) {
  // x = LN(x + MHA(x)); x = LN(x + FFN(x))          amt_apc.py:244-259
  if (S % 64 == 0 && M % 32 == 0) {
    ProjArgs pa = {};
    pa.X = X; pa.ldx = 256; pa.M = M; pa.nblk = 3; pa.S = S; pa.kv_nstep = S / 64;
    pa.blk[0] = pblock(w.pq, w.qkv.b, PROJ_ROW, e->QK, 256);
    pa.blk[1] = pblock(w.pk, w.qkv.b + 256, PROJ_KFRAG, e->KVimg, 0);
    pa.blk[2] = pblock(w.pv, w.qkv.b + 512, PROJ_VFRAG, e->KVimg, 0);
    ETD_TRY(launch_proj256(pa, st));
    AttnFragArgs f = {};
    f.Q = e->QK; f.ldq = 256; f.q_seq_stride = (long long)S * 256; f.KV = e->KVimg;
    f.O = e->AO; f.ldo = 256; f.o_seq_stride = (long long)S * 256; f.n_seq = n_seq; f.Sq = S; f.Sk = S; f.scale_log2e = kScaleLog2e;
    ETD_TRY(launch_attn_frag(f, st));
  } else {
    const int Spad = ((S + 63) / 64) * 64;
    ETD_TRY(proj_qkv(X, M, w.pq, w.pk, w.pv, w.qkv.b, e->QK, e->VT, S, Spad, st));
    AttnArgs t = {};
    t.Q = e->QK; t.ldq = 512; t.q_seq_stride = (long long)S * 512;
    t.K = e->QK + 256; t.ldk = 512; t.k_seq_stride = (long long)S * 512;
    t.VT = e->VT; t.Spad = Spad;
    t.O = e->AO; t.ldo = 256; t.o_seq_stride = (long long)S * 256;
    t.n_seq = n_seq; t.Sq = S; t.Sk = S; t.scale_log2e = kScaleLog2e;
    ETD_TRY(launch_attn(t, st));
  }
  ETD_TRY(proj_ln(e->AO, M, w.po, w.o.b, X, 0, w.g, w.be, X1, st));
  FfnArgs f = {X1, w.ffn, w.f1.b, w.f2.b, w.g, w.be, Yfinal, M};
  return launch_ffn_fused(f, st);
}

struct Outs { float *on, *off, *mpe; int8_t* vel; };

int tap(etd_ext* e, int stage, const void* src, size_t bytes, bool first, hipStream_t st) {
  if (first && e->tap[stage]) HIP_TRY(hipMemcpyAsync(e->tap[stage], src, bytes, hipMemcpyDeviceToDevice, st));
  return ETD_OK;
}

// windows [w0, w0+nw) of the current call; src describes where their input lives
int run_window_batch(etd_ext* e, const EmbedArgs& src_tmpl, int w0, int nw, long long out_row0, Outs B, Outs A, bool wantA, hipStream_t st) {
  const int nf = e->nf, nn = e->nn;
  for (int f0 = 0; f0 < nf; f0 += e->fc) {
    const int fc = (nf - f0) < e->fc ? (nf - f0) : e->fc;
    const int Mtok = nw * fc * 256, Mq = nw * fc * nn, nfr = nw * fc;
    // ---- encoder (amt_apc.py:74-120)
    EmbedArgs ea = src_tmpl;
    ea.Wf = e->Wf; ea.bf = e->bfold; ea.pos = e->pos_freq_enc; ea.Y = e->X; ea.w0 = w0; ea.n_win = nw; ea.f0 = f0; ea.fc = fc;
    ea.nf = nf; ea.margin = e->margin; ea.center = -8.0f; ea.pad_value = e->cfg.min_value;
    ETD_TRY(launch_embed(ea, st));
    const bool first = (w0 == 0 && f0 == 0);
    ETD_TRY(tap(e, 0, e->X, (size_t)Mtok * 512, first, st));
    for (int l = 0; l < 3; ++l) {
      const EncLayerW& w = e->enc[l];
      EncLayerArgs la = {e->X, w.lw, w.qkv.b, w.o.b, w.g, w.be, w.f1.b, w.f2.b, e->X, nfr};
      ETD_TRY(launch_enc_layer(la, st));
      ETD_TRY(tap(e, 1 + l, e->X, (size_t)Mtok * 512, first, st));
    }
    // ---- cross-attention K/V of the encoder output for the 3 decoder layers as MFMA-fragment images, in ONE launch: six blocks over the same token tile
    {
      ProjArgs pa = {};
      pa.X = e->X; pa.ldx = 256; pa.M = Mtok; pa.nblk = 6; pa.S = 256; pa.Spad = 256; pa.kv_nstep = 4;
      for (int l = 0; l < 3; ++l) {
        pa.blk[2 * l] = pblock(e->dec[l].pkc, e->bkv_all + l * 512, PROJ_KFRAG, e->KVcimg + (size_t)l * e->MTe * 512, 0);
        pa.blk[2 * l + 1] = pblock(e->dec[l].pvc, e->bkv_all + l * 512 + 256, PROJ_VFRAG, e->KVcimg + (size_t)l * e->MTe * 512, 0);
      }
      ETD_TRY(launch_proj256(pa, st));
    }
    // ---- frequency decoder (amt_apc.py:168-177,261-320): queries = 88 note embeddings per frame
    // D0 = layer input/output, D1 = after self-attention LN, D2 = after cross-attention LN
    e16 *D0 = e->Tq, *D1 = e->T1, *D2 = e->Tfreq;
    for (int l = 0; l < 3; ++l) {
      const DecLayerW& w = e->dec[l];
      const e16* cross_in = D0;        // residual + query source of the cross-attention block
      int r_mod = 0;
      if (l == 0) { cross_in = e->trg0; r_mod = nn; }
      if (w.has_self) {
        ETD_TRY(proj_qkv(D0, Mq, w.pq, w.pk, w.pv, w.qkv_s.b, e->QKd, e->VTd, nn, 128, st));
        AttnArgs t = {};
        t.Q = e->QKd; t.ldq = 512; t.q_seq_stride = (long long)nn * 512;
        t.K = e->QKd + 256; t.ldk = 512; t.k_seq_stride = (long long)nn * 512;
        t.VT = e->VTd; t.Spad = 128; t.O = e->AOd; t.ldo = 256; t.o_seq_stride = (long long)nn * 256;
        t.n_seq = nfr; t.Sq = nn; t.Sk = nn; t.scale_log2e = kScaleLog2e;
        ETD_TRY(launch_attn(t, st));
        ETD_TRY(proj_ln(e->AOd, Mq, w.po, w.o_s.b, D0, 0, w.g, w.be, D1, st));
        cross_in = D1;
      }
      AttnFragArgs f = {};
      if (l == 0) {
        f.Q = e->q0; f.ldq = 256; f.q_seq_stride = 0;       // constant queries, precomputed at load
      } else {
        ProjArgs pa = {};
        pa.X = cross_in; pa.ldx = 256; pa.M = Mq; pa.nblk = 1;
        pa.blk[0] = pblock(w.pqc, w.q_c.b, PROJ_ROW, e->Qd, 256);
        ETD_TRY(launch_proj256(pa, st));
        f.Q = e->Qd; f.ldq = 256; f.q_seq_stride = (long long)nn * 256;
      }
      f.KV = e->KVcimg + (size_t)l * e->MTe * 512;
      f.O = e->AOd; f.ldo = 256; f.o_seq_stride = (long long)nn * 256; f.n_seq = nfr; f.Sq = nn; f.Sk = 256; f.scale_log2e = kScaleLog2e;
      ETD_TRY(launch_attn_frag(f, st));
      ETD_TRY(proj_ln(e->AOd, Mq, w.poc, w.o_c.b, cross_in, r_mod, w.g, w.be, D2, st));
      FfnArgs ff = {D2, w.ffn, w.f1.b, w.f2.b, w.g, w.be, D0, Mq};
      ETD_TRY(launch_ffn_fused(ff, st));
      ETD_TRY(tap(e, 4 + l, D0, (size_t)Mq * 512, first, st));
    }
    // freq -> time layout of this chunk, *16 + pos_embedding_time (amt_apc.py:203-205); optional A heads (:186-189)
    ETD_TRY(launch_freq2time(D0, e->TI, e->pos_time, nw, fc, f0, nf, nn, st));
    if (wantA) {
      for (int wl = 0; wl < nw; ++wl) {
        HeadsArgs h = {};
        h.X = D0 + (size_t)wl * fc * nn * 256; h.W = e->head_freq.W; h.bias = e->head_freq.b; h.M = fc * nn; h.time_layout = 0;
        h.nf = nf; h.nn = nn; h.out_off = out_row0 * nn + ((long long)wl * nf + f0) * nn;
        h.onset = A.on; h.offset = A.off; h.mpe = A.mpe; h.vel = A.vel;
        ETD_TRY(launch_heads(h, st));
      }
    }
  }
  // ---- time decoder (amt_apc.py:211-220): nw*nn sequences of nf frames
  const int Mt = nw * nn * nf;
  ETD_TRY(tap(e, 7, e->TI, (size_t)Mt * 512, w0 == 0, st));
  for (int l = 0; l < 3; ++l) {
    ETD_TRY(enc_like_layer(e, e->tim[l], e->TI, e->X1, Mt, nw * nn, nf, st, e->TI));
    ETD_TRY(tap(e, 8 + l, e->TI, (size_t)Mt * 512, w0 == 0, st));
  }
  HeadsArgs h = {};
  h.X = e->TI; h.W = e->head_time.W; h.bias = e->head_time.b; h.M = Mt; h.time_layout = 1; h.nf = nf; h.nn = nn;
  h.out_off = out_row0 * nn;
  h.onset = B.on; h.offset = B.off; h.mpe = B.mpe; h.vel = B.vel;
  h.vel_logit = e->dbg_vel;            // (the kernel's output index already carries out_off)
  ETD_TRY(launch_heads(h, st));
  return ETD_OK;
}

int run_all(etd_ext* e, EmbedArgs src, int n_windows, Outs B, Outs A, hipStream_t st) {
  if (e->f32) return ext32_run(e->f32, src, n_windows, Outs32{B.on, B.off, B.mpe, B.vel}, Outs32{A.on, A.off, A.mpe, A.vel}, e->tap, e->dbg_vel, st);
  const bool wantA = A.on && A.off && A.mpe && A.vel;
  for (int w0 = 0; w0 < n_windows; w0 += e->wb) {
    const int nw = (n_windows - w0) < e->wb ? (n_windows - w0) : e->wb;
    ETD_TRY(run_window_batch(e, src, w0, nw, (long long)w0 * e->nf, B, A, wantA, st));
  }
  return ETD_OK;
}

}  // namespace

extern "C" int etd_transcript(etd_ext* e, const float* feat_dev, long long T, float* onset_B, float* offset_B, float* mpe_B,
                              int8_t* vel_B, float* onset_A, float* offset_A, float* mpe_A, int8_t* vel_A, void* stream) {
  if (!e || !feat_dev || T <= 0 || !onset_B || !offset_B || !mpe_B || !vel_B) ETD_FAIL(ETD_EINVAL, "transcript: bad args");
  EmbedArgs s = {};
  s.src = feat_dev; s.feat_mode = 1; s.T = T; s.s_t = e->cfg.n_bin; s.s_bin = 1; s.s_win = 0;
  const int nwin = (int)((T + e->nf - 1) / e->nf);
  return run_all(e, s, nwin, Outs{onset_B, offset_B, mpe_B, vel_B}, Outs{onset_A, offset_A, mpe_A, vel_A}, (hipStream_t)stream);
}

extern "C" int etd_transcript_windows(etd_ext* e, const float* spec_dev, int B, float* onset_B, float* offset_B, float* mpe_B,
                                      int8_t* vel_B, float* onset_A, float* offset_A, float* mpe_A, int8_t* vel_A, void* stream) {
  if (!e || !spec_dev || B <= 0 || !onset_B || !offset_B || !mpe_B || !vel_B) ETD_FAIL(ETD_EINVAL, "transcript_windows: bad args");
  EmbedArgs s = {};
  const long long nin = e->nf + 2 * e->margin;
  s.src = spec_dev; s.feat_mode = 0; s.s_win = (long long)e->cfg.n_bin * nin; s.s_bin = nin; s.s_t = 1;
  return run_all(e, s, B, Outs{onset_B, offset_B, mpe_B, vel_B}, Outs{onset_A, offset_A, mpe_A, vel_A}, (hipStream_t)stream);
}

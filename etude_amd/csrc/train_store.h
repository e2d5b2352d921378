// The part of a trainer that has nothing to do with its model ("trainer skeleton"): the named tensors of the flat [P | G | M1 | M2] buffers, the
// host image filled from a checkpoint, the gradient norm, the step counter, the clipped AdamW step and the host's checked access to one named tensor.  A handle
// holds one TrainStore by value; its extern "C" entries are a null check plus one call.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "host_util.h"
#include "prof.h"
#include "train_kernels.h"

struct TrainStore {
  struct Tensor { std::string name; size_t off, n; };
  std::vector<Tensor> tensors;
  std::map<std::string, int> index;                    // name -> position in `tensors`
  size_t n_total = 0, n_train = 0;                     // floats of P; the first n_train are trained (the engine sets n_train once its trained tensors are added)
  float *P = nullptr, *G = nullptr, *M1 = nullptr, *M2 = nullptr;
  double* partial = nullptr;                           // [TN_BLOCKS], the norm's partial sums (allocated by the engine from its pool)
  long long step = 0;

  // the next tensor, on a 256-byte boundary; the gaps stay 0 in all four buffers.  Returns its offset
  size_t add(const std::string& name, size_t n) {
    const size_t off = n_total;
    add_at(name, off, n);
    n_total += (n + 63) / 64 * 64;
    return off;
  }
  // a tensor at an offset the engine chose (a slice of a packed layout: no padding, n_total is the engine's)
  void add_at(const std::string& name, size_t off, size_t n) {
    index[name] = (int)tensors.size();
    tensors.push_back({name, off, n});
  }

  // host [n_total] <- every tensor from the checkpoint; a missing or wrongly sized one fails with the table's message
  int fill(const WeightTable& wt, float* host) const {
    for (const Tensor& t : tensors) {
      const float* src = wt.get(t.name, (int64_t)t.n);
      if (!src) return ETD_EINVAL;
      memcpy(host + t.off, src, t.n * sizeof(float));
    }
    return ETD_OK;
  }
  // P <- host [n_total]; G, M1, M2 [n_grad] zeroed
  int upload(DevPool& pl, const float* host, size_t n_grad) {
    ETD_TRY((pl.upload<float, float>(&P, host, n_total)));
    ETD_TRY(pl.alloc(&G, n_grad, true));
    ETD_TRY(pl.alloc(&M1, n_grad, true));
    return pl.alloc(&M2, n_grad, true);
  }

  int zero_grad(size_t count, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(G, 0, sizeof(float) * count, st));
    return ETD_OK;
  }
  int grad_norm(size_t count, hipStream_t st, double* out) { return ::grad_norm(G, (long long)count, partial, st, out); }

  // the tensor `name` of exactly `numel` elements, or a refusal (`what`: the engine's word for an entry, "parameter" or "tensor")
  int find(const char* who, const char* what, const char* name, long long numel, const Tensor** out) const {
    auto it = index.find(name);
    if (it == index.end()) ETD_FAIL(ETD_EINVAL, "%s: no %s '%s'", who, what, name);
    const Tensor& t = tensors[it->second];
    if ((long long)t.n != numel) ETD_FAIL(ETD_EINVAL, "%s: '%s' has %zu elements, the buffer %lld", who, name, t.n, numel);
    *out = &t;
    return ETD_OK;
  }
  // one tensor of a flat buffer to the host (`out`) or from it (`in`).  which: 0 parameter (state), 1 gradient, 2 exp_avg, 3 exp_avg_sq
  int copy(const Tensor& t, int which, float* out, const float* in, hipStream_t st) {
    float* base = (which == 0 ? P : which == 1 ? G : which == 2 ? M1 : M2) + t.off;
    if (out) HIP_TRY(hipMemcpyAsync(out, base, sizeof(float) * t.n, hipMemcpyDeviceToHost, st));
    else HIP_TRY(hipMemcpyAsync(base, in, sizeof(float) * t.n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return ETD_OK;
  }
};

// The host's read (`out`) or write (`in`) of one named tensor, with the checks every trainer makes; `s` is null when the caller's handle is
inline int train_io(TrainStore* s, const char* who, const char* name, int which, float* out, const float* in, long long numel, hipStream_t st) {
  if (!s || !name || (!out && !in)) ETD_FAIL(ETD_EINVAL, "%s: null argument", who);
  const TrainStore::Tensor* t = nullptr;
  ETD_TRY(s->find(who, "parameter", name, numel, &t));
  return s->copy(*t, which, out, in, st);
}

// clip_grad_norm_ and torch.optim.AdamW's step over the first `count` floats: the norm, step += 1, k_tadamw (`who`: the entry's name in a refusal, `scope`: its
// name in a profile)
inline int adamw_step(TrainStore& s, size_t count, const char* who, const char* scope, double max_norm, double lr, double beta1, double beta2, double eps,
                      double weight_decay, double* norm_out, hipStream_t st) {
  ETD_TRY(adamw_check(who, lr, beta1, beta2, eps, weight_decay));
  ProfScope ps(scope, st);
  double norm = 0.0;
  ETD_TRY(s.grad_norm(count, st, &norm));
  if (norm_out) *norm_out = norm;
  s.step += 1;
  launch_tadamw(s.P, s.G, s.M1, s.M2, (long long)count, adamw_args(max_norm, norm, lr, beta1, beta2, eps, weight_decay, s.step), st);
  HIP_TRY(hipGetLastError());
  return ETD_OK;
}

// numpy's add.reduce over contiguous doubles, restated for one lane (or the host): the order DESIGN.md 4h and 4i fix for every mean they take.
#pragma once

#pragma clang fp contract(off)      // (and for the rest of the including file: every user of these sums rounds each operation on its own)

#define NP_SUM_HD __host__ __device__ __forceinline__

// ... over n <= 128 doubles a(i): below 8 sequential, else eight accumulators over whole groups of 8, combined pairwise, then the remainder
template <class F>
NP_SUM_HD double np_sum_leaf(int n, F a) {
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res += a(i);
    return res;
  }
  double r0 = a(0), r1 = a(1), r2 = a(2), r3 = a(3), r4 = a(4), r5 = a(5), r6 = a(6), r7 = a(7);
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 += a(i); r1 += a(i + 1); r2 += a(i + 2); r3 += a(i + 3); r4 += a(i + 4); r5 += a(i + 5); r6 += a(i + 6); r7 += a(i + 7);
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) res += a(i);
  return res;
}

// ... over any n: above 128 split at n / 2 rounded down to a multiple of 8, left + right (the recursion unrolled onto a small stack; one lane runs it)
template <class F>
NP_SUM_HD double np_sum_all(int n, F a) {
  struct Fr { int off, n, stage; double left; };
  Fr st[20];
  int sp = 0;
  st[sp].off = 0; st[sp].n = n; st[sp].stage = 0; st[sp].left = 0.0; ++sp;
  double ret = 0.0;
  while (sp > 0) {
    Fr& f = st[sp - 1];
    if (f.stage == 0) {
      if (f.n <= 128) {
        const int off = f.off;
        ret = np_sum_leaf(f.n, [&](int i) { return a(off + i); });
        --sp;
        continue;
      }
      int n2 = f.n / 2; n2 -= n2 % 8;
      f.stage = 1;
      st[sp].off = f.off; st[sp].n = n2; st[sp].stage = 0; st[sp].left = 0.0; ++sp;
    } else if (f.stage == 1) {
      int n2 = f.n / 2; n2 -= n2 % 8;
      f.left = ret; f.stage = 2;
      st[sp].off = f.off + n2; st[sp].n = f.n - n2; st[sp].stage = 0; st[sp].left = 0.0; ++sp;
    } else {
      ret = f.left + ret;
      --sp;
    }
  }
  return ret;
}

// The body of skinny_fwd_kernel<KV, W_KC, EPI> (skinny.hip), included into the lone kernel
// and into its member-indexed twin: ONE text, compiled in each kernel's own function, so
// that the lone kernel's code is what it was before the twin existed.  Reads: p (a
// SkinnyFwdParams), KV / W_KC / EPI, and the workgroup's (blockIdx.x, blockIdx.y) as the
// row block and column block of ITS product.
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [rows][4 KV]
  const int tid = threadIdx.x;
  const int q = tid % p.qpr;                 // column quad inside the block
  const int rg = tid / p.qpr;                // row group
  const int n_rg = SK_THREADS / p.qpr;
  const int n0 = (blockIdx.y * p.qpr + q) * 4;
  const bool col_ok = n0 < p.N;              // N % 4 == 0
  const int nc = col_ok ? n0 : 0;
  const int rows_per_block = n_rg * p.rows_per_thread;
  const int row0 = blockIdx.x * rows_per_block;
  const int row_end = min(p.M, row0 + rows_per_block);

  // ---- stage the block's X rows (columns >= K zeroed: the padding may hold
  // anything, and 0 * NaN would poison the sums)
  for (int i = tid; i < rows_per_block * KV; i += SK_THREADS) {
    const int r = i / KV, v = i % KV;
    const int m = min(row0 + r, p.M - 1);
    const int64_t src = p.idx ? (int64_t)p.idx[m] : (int64_t)m;
    float4 x = *reinterpret_cast<const float4*>(p.X + src * p.ldx + 4 * v);
    x.x = (4 * v + 0 < p.K) ? x.x : 0.f;
    x.y = (4 * v + 1 < p.K) ? x.y : 0.f;
    x.z = (4 * v + 2 < p.K) ? x.z : 0.f;
    x.w = (4 * v + 3 < p.K) ? x.w : 0.f;
    *reinterpret_cast<float4*>(xs + (r * KV + v) * 4) = x;
  }

  // wk[k] = W(n0..n0+3, k)
  float4 wk[4 * KV];
  if (W_KC) {
#pragma unroll
    for (int v = 0; v < KV; ++v) {
      float4 r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        r[j] = *reinterpret_cast<const float4*>(p.W + (int64_t)(nc + j) * p.ldw + 4 * v);
      wk[4 * v + 0] = make_float4(r[0].x, r[1].x, r[2].x, r[3].x);
      wk[4 * v + 1] = make_float4(r[0].y, r[1].y, r[2].y, r[3].y);
      wk[4 * v + 2] = make_float4(r[0].z, r[1].z, r[2].z, r[3].z);
      wk[4 * v + 3] = make_float4(r[0].w, r[1].w, r[2].w, r[3].w);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4 * KV; ++k)
      wk[k] = *reinterpret_cast<const float4*>(p.W + (int64_t)min(k, p.K - 1) * p.ldw + nc);
  }
  float4 bias = make_float4(0.f, 0.f, 0.f, 0.f);
  if (EPI == 0 && p.bias) bias = *reinterpret_cast<const float4*>(p.bias + nc);
  __syncthreads();

  for (int it = 0; it < p.rows_per_thread; it += SK_UNROLL) {
    float4 h[SK_UNROLL];
    if (EPI == 1) {
#pragma unroll
      for (int u = 0; u < SK_UNROLL; ++u) {
        const int m = min(row0 + (it + u) * n_rg + rg, p.M - 1);
        h[u] = *reinterpret_cast<const float4*>(p.H + (int64_t)m * p.ldh + nc);
      }
    }
#pragma unroll
    for (int u = 0; u < SK_UNROLL; ++u) {
      const int rl = (it + u) * n_rg + rg;
      const int m = row0 + rl;
      // two packed FMAs (v_pk_fma_f32) per k instead of four scalar ones: the same
      // fmaf chain per output, half the vector-issue slots
      const float4 a0 = (EPI == 0) ? bias : make_float4(0.f, 0.f, 0.f, 0.f);
      sk_v2f alo = {a0.x, a0.y}, ahi = {a0.z, a0.w};
#pragma unroll
      for (int v = 0; v < KV; ++v) {
        const float4 xv = *reinterpret_cast<const float4*>(xs + (rl * KV + v) * 4);
        const float xk[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float4 w = wk[4 * v + j];
          const sk_v2f xx = {xk[j], xk[j]};
          const sk_v2f wlo = {w.x, w.y}, whi = {w.z, w.w};
          alo = __builtin_elementwise_fma(xx, wlo, alo);
          ahi = __builtin_elementwise_fma(xx, whi, ahi);
        }
      }
      float4 a = make_float4(alo.x, alo.y, ahi.x, ahi.y);
      if (EPI == 0) {
        if (p.act == 1) {
          a.x = tanh_fast(a.x); a.y = tanh_fast(a.y);
          a.z = tanh_fast(a.z); a.w = tanh_fast(a.w);
        }
      } else {
        a.x *= (1.f - h[u].x * h[u].x);
        a.y *= (1.f - h[u].y * h[u].y);
        a.z *= (1.f - h[u].z * h[u].z);
        a.w *= (1.f - h[u].w * h[u].w);
      }
      if (m < row_end && col_ok)
        *reinterpret_cast<float4*>(p.Y + (int64_t)m * p.ldy + n0) = a;
    }
  }

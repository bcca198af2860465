// The bodies of the loss and KL row kernels of losses.hip, one per value of GA_LOSS_BODY,
// included into the lone kernel and into its member-indexed twin (members_diag.h): ONE
// text, compiled in each kernel's own function, so that the lone kernel's code is what it
// was before the twin existed.  A body reads its kernel's parameters by their names (p, or
// the scalar arguments of the KL kernels), the block index blockIdx.x, and the block count
// GA_GRID_X: gridDim.x in the lone kernel, the entry's own block count in the twin.
//   1 ppo_gaussian_loss_kernel   2 ppo_categorical_loss_kernel   3 categorical_kl_kernel
//   4 gaussian_nll_kernel        5 gaussian_kl_kernel
#if GA_LOSS_BODY == 1  // ppo_gaussian_loss_kernel
  __shared__ double red[4];
  const float s = ga_log_std(*p.log_std, p.has_min, p.min_log_std, p.has_max,
                             p.max_log_std, nullptr);
  const float inv_var = expf(-2.f * s);
  const float lognorm = s + (float)HALF_LOG_2PI;
  const float invM = 1.f / (float)p.M;

  double obj_sum = 0.0, ds_sum = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.M;
       i += (int64_t)GA_GRID_X * 256) {
    const int64_t src = p.idx ? (int64_t)p.idx[i] : i;
    const float* mu = p.mean + i * p.ldm;
    const float* a = p.actions + src * p.lda;
    float ll = 0.f, q = 0.f;  // q = sum (a-mu)^2 / var
    for (int j = 0; j < p.A; ++j) lr_gauss_dim(a[j], mu[j], inv_var, lognorm, q, ll);
    if (p.ll_out) p.ll_out[i] = ll;
    float g;  // d obj / d ll
    const float obj = lr_surrogate(p.algo, p.clip, ll, p.algo == 1 ? 0.f : p.old_ll[src],
                                   p.adv[src], &g);
    obj_sum += (double)obj;
    if (p.dmean) {
      float* dm = p.dmean + i * p.ldm;
      const float scale = -g * invM * inv_var;
      for (int j = 0; j < p.A; ++j) dm[j] = scale * (a[j] - mu[j]);
    }
    // d ll / d s = sum_j ((a-mu)^2/var - 1)
    ds_sum += (double)(-g * (q - (float)p.A));
  }
  const double o = ga_block_sum_256(obj_sum, red);
  const double d = ga_block_sum_256(ds_sum, red);
  double bo = o, bd = d;  // batch sums (the only block: its own)
  if (GA_GRID_X > 1 || !p.loss_out) {
    if (threadIdx.x == 0) {
      p.partials[2 * blockIdx.x + 0] = o;
      p.partials[2 * blockIdx.x + 1] = d;
    }
    if (!p.loss_out || !ga_take_last_ticket(p.ticket)) return;
    if (threadIdx.x >= 64) return;
    bo = ga_sum_partials(p.partials, GA_GRID_X, 0);
    bd = ga_sum_partials(p.partials, GA_GRID_X, 1);
  }
  if (threadIdx.x == 0 && p.loss_out)
    ppo_gaussian_finish(bo, bd, p.log_std, p.has_min, p.min_log_std, p.has_max,
                        p.max_log_std, p.M, p.A, p.ent, p.loss_out, p.grad_slab0,
                        p.slab_stride, p.n_splits);
#elif GA_LOSS_BODY == 2  // ppo_categorical_loss_kernel
  __shared__ double red[4];
  const float invM = 1.f / (float)p.M;
  double obj_sum = 0.0, ent_sum = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.M;
       i += (int64_t)GA_GRID_X * 256) {
    const int64_t src = p.idx ? (int64_t)p.idx[i] : i;
    const float* sc = p.scores + i * p.lds;
    const int a = (int)p.actions[src * p.lda];
    float lse, mx, den;
    cat_row(sc, p.A, p.double_softmax, &lse, &mx, &den);
    // log-prob of the taken action and the entropy H = -sum q lp
    float ll = 0.f, H = 0.f;
    for (int j = 0; j < p.A; ++j) {
      const float pj = expf(sc[j] - mx) / den;
      const float lp = (p.double_softmax ? pj : sc[j]) - lse;
      const float q = expf(lp);
      H -= q * lp;
      if (j == a) ll = lp;
    }
    float Hs = H, dHs = 1.f;  // softplus(H) and its derivative
    if (p.ent.softplus) Hs = lr_softplus(H, &dHs);
    if (p.ll_out) p.ll_out[i] = ll;
    if (p.ent_out) p.ent_out[i] = Hs;
    float g;
    float obj = lr_surrogate(p.algo, p.clip, ll, p.algo == 1 ? 0.f : p.old_ll[src],
                             p.adv[src], &g);
    if (p.ent.regularized) obj += p.ent.coeff * Hs;
    obj_sum += (double)obj;
    ent_sum += (double)Hs;
    if (p.dscores) {
      const float cH = (p.ent.regularized && !p.ent.stop_grad) ? p.ent.coeff * dHs : 0.f;
      float* ds = p.dscores + i * p.lds;
      if (!p.double_softmax) {
        for (int j = 0; j < p.A; ++j)
          ds[j] = -lr_cat_grad(g, cH, sc[j] - lse, H, j == a) * invM;
      } else {
        // chain through p = softmax(scores): dz_k = p_k (dp_k - sum_j dp_j p_j)
        float dot = 0.f;
        for (int j = 0; j < p.A; ++j) {
          const float pj = expf(sc[j] - mx) / den;
          dot += lr_cat_grad(g, cH, pj - lse, H, j == a) * pj;
        }
        for (int k = 0; k < p.A; ++k) {
          const float pk = expf(sc[k] - mx) / den;
          const float dp = lr_cat_grad(g, cH, pk - lse, H, k == a);
          ds[k] = -(pk * (dp - dot)) * invM;
        }
      }
    }
  }
  const double o = ga_block_sum_256(obj_sum, red);
  const double e = ga_block_sum_256(ent_sum, red);
  double bo = o, be = e;  // batch sums (the only block: its own)
  if (GA_GRID_X > 1 || !p.loss_out) {
    if (threadIdx.x == 0) {
      p.partials[2 * blockIdx.x + 0] = o;
      p.partials[2 * blockIdx.x + 1] = e;
    }
    if (!p.loss_out || !ga_take_last_ticket(p.ticket)) return;
    if (threadIdx.x >= 64) return;
    bo = ga_sum_partials(p.partials, GA_GRID_X, 0);
    be = ga_sum_partials(p.partials, GA_GRID_X, 1);
  }
  if (threadIdx.x == 0) {
    *p.loss_out = (float)(-(bo / (double)p.M));
    if (p.ent_sum_out) *p.ent_sum_out = be;
    if (p.grad_slab0)  // the (unused) log-std slot of the flat layout stays 0
      for (int64_t k = 0; k < p.n_splits; ++k) p.grad_slab0[k * p.slab_stride] = 0.f;
  }
#elif GA_LOSS_BODY == 3  // categorical_kl_kernel
  __shared__ double red[4];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M;
       i += (int64_t)GA_GRID_X * 256) {
    const float* so = sc_old + i * ld;
    const float* sn = sc_new + i * ld;
    float lo, mo, den_o, ln, mn, dn;
    cat_row(so, A, dbl, &lo, &mo, &den_o);
    cat_row(sn, A, dbl, &ln, &mn, &dn);
    float kl = 0.f;
    for (int j = 0; j < A; ++j) {
      const float lpo = (dbl ? expf(so[j] - mo) / den_o : so[j]) - lo;
      const float lpn = (dbl ? expf(sn[j] - mn) / dn : sn[j]) - ln;
      kl += expf(lpo) * (lpo - lpn);
    }
    acc += (double)kl;
  }
  const double r = ga_block_sum_256(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = r;
#elif GA_LOSS_BODY == 4  // gaussian_nll_kernel
  __shared__ double red[4];
  const float s = *p.log_std;
  const float inv_var = expf(-2.f * s);
  const float invM = 1.f / (float)p.M;
  double nll = 0.0, ds = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.M;
       i += (int64_t)GA_GRID_X * 256) {
    const int64_t src = p.idx ? (int64_t)p.idx[i] : i;
    float dsi, dvi;
    nll += (double)lr_nll_row(p.returns[src], p.v[i * p.ldv], s, inv_var, invM, &dsi, &dvi);
    ds += (double)dsi;
    if (p.dv) p.dv[i * p.ldv] = dvi;
  }
  const double a = ga_block_sum_256(nll, red);
  const double b = ga_block_sum_256(ds, red);
  double ba = a, bb = b;  // batch sums (the only block: its own)
  if (GA_GRID_X > 1 || !p.loss_out) {
    if (threadIdx.x == 0) {
      p.partials[2 * blockIdx.x + 0] = a;
      p.partials[2 * blockIdx.x + 1] = b;
    }
    if (!p.loss_out || !ga_take_last_ticket(p.ticket)) return;
    if (threadIdx.x >= 64) return;
    ba = ga_sum_partials(p.partials, GA_GRID_X, 0);
    bb = ga_sum_partials(p.partials, GA_GRID_X, 1);
  }
  if (threadIdx.x == 0 && p.loss_out) {
    *p.loss_out = (float)(ba / (double)p.M);
    if (p.grad_slab0) {
      p.grad_slab0[0] = (float)(bb / (double)p.M);
      for (int64_t k = 1; k < p.n_splits; ++k) p.grad_slab0[k * p.slab_stride] = 0.f;
    }
  }
#elif GA_LOSS_BODY == 5  // gaussian_kl_kernel
  __shared__ double red[4];
  // torch kl_normal_normal: 0.5 * (var_ratio + t1 - 1 - log(var_ratio))
  const float ratio = expf(s_old - s_new);
  const float var_ratio = ratio * ratio;
  const float inv_std_new = expf(-s_new);
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M;
       i += (int64_t)GA_GRID_X * 256) {
    float kl = 0.f;
    for (int j = 0; j < A; ++j) {
      const float t = (mean_old[i * ld + j] - mean_new[i * ld + j]) * inv_std_new;
      kl += 0.5f * (var_ratio + t * t - 1.f - logf(var_ratio));
    }
    acc += (double)kl;
  }
  const double r = ga_block_sum_256(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = r;
#else
#error "GA_LOSS_BODY must be 1 .. 5"
#endif

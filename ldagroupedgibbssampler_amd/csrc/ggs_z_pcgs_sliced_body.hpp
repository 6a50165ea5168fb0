// ggs_z_pcgs_sliced_body.hpp -- the body of pcgs_sliced_kernel<KMAX, COLLAPSED> and polyaurn_sliced_kernel<KMAX>
// (ggs_z_pcgs.hpp), included INSIDE each kernel with the constants KMAX, COLLAPSED and POLYAURN in scope.  Not a
// function: the same code behind a device-function call changed pcgs_sliced_kernel's register allocation (a few AGPRs at
// KMAX = 96 and 112), and the pcgs instances are to compile exactly as they did before scheme polyaurn existed.
// No include guard on purpose.
  constexpr int NS = (KMAX + kSliceTopics - 1) / kSliceTopics;
  constexpr int kAhead = NS < kPcgsRingSlots - 1 ? NS : kPcgsRingSlots - 1;
  constexpr int kHead = pcgs_sliced_head_bytes(KMAX);              // alpha row + counts, below the ring (>= NS*128)
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x;
  const int K = p.K;
  double *alb = reinterpret_cast<double *>(smem);                  // alpha, zero padded to KMAX
  int16_t *cnt = reinterpret_cast<int16_t *>(smem + KMAX * 8);     // [KMAX][64]
  unsigned char *ring = smem + kHead;
  const unsigned char *phib = reinterpret_cast<const unsigned char *>(p.phiT);
  const size_t rowbytes = (size_t)p.Kp * 8;
  const int lrow = lane >> 3, lslot = lane & 7;
  const unsigned char *my_row = ring + lane * 128;
  const int rot = lane >> 1;
  const int16_t *my_cnt = cnt + lane;

  auto row_addresses = [&](const int w, const unsigned char *(&ra)[8]) {
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int row = 8 * m + lrow;
      const int wm = __shfl(w, row);
      ra[m] = phib + (size_t)wm * rowbytes + (size_t)(((lslot - (row >> 1)) & 7) << 4);
    }
  };
  auto issue_slice = [&](auto sc, const int slot, const unsigned char *const (&ra)[8]) {
    constexpr int s = decltype(sc)::value;
#pragma unroll
    for (int m = 0; m < 8; ++m)
      __builtin_amdgcn_global_load_lds((glb_cvoid_t *)ra[m], (lds_void_t *)(ring + slot * kSliceBytes + m * 1024 - s * 128), 16, s * 128, 0);
  };

  for (int k = lane; k < KMAX; k += 64) alb[k] = k < K ? p.alpha[k] : 0.0;

  const int64_t groups = (p.num_docs + 63) / 64;
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t di = g * 64 + lane;
    const int d = di < p.num_docs ? p.order[di] : -1;
    const int64_t beg = d >= 0 ? p.doc_ptr[d] : 0;
    const int len = d >= 0 ? (int)(p.doc_ptr[d + 1] - beg) : 0;
    const int steps = __shfl(len, 0);                              // lane 0 holds the group's longest document
    if (steps == 0) break;                                         // sorted: every later group is empty too
    for (int k = 0; k < KMAX; ++k) cnt[k * 64 + lane] = 0;         // UPLDA:1482-1485 localTopicCounts
    for (int t = 0; t < len; ++t) cnt[p.z[beg + t] * 64 + lane] += 1;

    int w = len > 0 ? p.tok[beg] : 0;
    const unsigned char *ra[8], *ran[8];
    row_addresses(w, ra);
    int gs = 0;
    static_for<0, kAhead>([&](auto sc) { issue_slice(sc, decltype(sc)::value % kPcgsRingSlots, ra); });
    int znext = len > 0 ? p.z[beg] : 0;                            // old topic and (COLLAPSED) its own-token psi, one step ahead (see pcgs_z_kernel)
    auto own_of = [&](const int word, const int topic) {
      return (p.beta + (double)(p.n_wk[(size_t)word * K + topic] - 1)) / (p.beta_sum + (double)(p.n_k[topic] - 1));
    };
    double own_next = (COLLAPSED && len > 0) ? own_of(w, znext) : 0.0;

    for (int t = 0; t < steps; ++t) {
      const bool active = t < len, has1 = t + 1 < steps;
      gs = __builtin_amdgcn_readfirstlane(gs);
      const int zold = znext;
      const double own = own_next;
      const int ip = active ? p.inv_perm[beg + t] : 0;
      const int w1 = (t + 1 < len) ? p.tok[beg + t + 1] : 0;
      znext = (t + 1 < len) ? p.z[beg + t + 1] : 0;
      if (COLLAPSED && t + 1 < len) own_next = own_of(w1, znext);
      if (has1) row_addresses(w1, ran);
      if (active) cnt[zold * 64 + lane] -= 1;                      // UPLDA:1494
      asm volatile("" ::: "memory");

      double sc[KMAX];
      double sum = 0.0;
      static_for<0, NS>([&](auto sidx) {                           // UPLDA:1509-1513
        constexpr int s = decltype(sidx)::value;
        const int cur = (gs + s) % kPcgsRingSlots;
        const int nxt = (gs + s + kAhead) % kPcgsRingSlots;
        if constexpr (s + kAhead < NS) issue_slice(std::integral_constant<int, s + kAhead>{}, nxt, ra);
        else if (has1) issue_slice(std::integral_constant<int, s + kAhead - NS>{}, nxt, ran);
        if (has1 || s + kAhead < NS) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(8 * kAhead) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(8 * (NS - 1 - s)) : "memory");
        if (active) {
          const unsigned char *rb = my_row + cur * kSliceBytes;
          D2 ph[kSliceUnits], al[kSliceUnits];
          int n[kSliceTopics];
#pragma unroll
          for (int u = 0; u < kSliceUnits; ++u)
            if (s * kSliceTopics + 2 * u + 1 < KMAX) {
              ph[u] = lds_d2(rb + (((u + rot) & 7) << 4));
              al[u] = lds_d2(reinterpret_cast<const unsigned char *>(alb) + (s * kSliceTopics + 2 * u) * 8);
              n[2 * u] = my_cnt[(s * kSliceTopics + 2 * u) * 64];
              n[2 * u + 1] = my_cnt[(s * kSliceTopics + 2 * u + 1) * 64];
            }
          if constexpr (COLLAPSED) {
            const int rel = zold - s * kSliceTopics;               // position of the old topic inside this slice, if any
#pragma unroll
            for (int u = 0; u < kSliceUnits; ++u) {
              if (rel == 2 * u) ph[u].a = own;
              if (rel == 2 * u + 1) ph[u].b = own;
            }
          }
#pragma unroll
          for (int u = 0; u < kSliceUnits; ++u) {
            constexpr int k0 = s * kSliceTopics;
            const int k = k0 + 2 * u;
            if (k + 1 < KMAX) {
              sc[k] = ((double)n[2 * u] + al[u].a) * ph[u].a;
              sum += sc[k];
              sc[k + 1] = ((double)n[2 * u + 1] + al[u].b) * ph[u].b;
              sum += sc[k + 1];
            }
          }
        }
        asm volatile("" ::: "memory");
      });
      gs = (gs + NS) % kPcgsRingSlots;

      if (active) {
        const uint64_t gtok = (uint64_t)(p.tok_base + beg + t);
        const U4 o = philox4x32_10((uint32_t)gtok, (uint32_t)(gtok >> 32), (uint32_t)GGS_PURPOSE_Z << 24, p.iteration,
                                   (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
        double tt = 0.0 - u53(o.x, o.y) * sum;                     // UPLDA:1519-1526, negated walk (see ggs_z_sliced.hpp)
        if constexpr (POLYAURN)                                    // decided before the walk (pcgs_z_body): a walk from +0 stops at once
          if (len == 1 || sum == 0.0) tt = 0.0;
        int newc = 0;
        bool live = true;
#pragma unroll
        for (int kb = 0; kb < KMAX; kb += 16) {
          if (live) {
            uint32_t bits = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j)
              if (kb + j < KMAX) {
                bits = __builtin_amdgcn_alignbit(bits, (uint32_t)hi32(tt), 31);
                tt += sc[kb + j];
              }
            newc += __popc(bits);
            live = __any(hi32(tt) < 0);
          }
        }
        int new_topic = newc - 1;
        if (POLYAURN && (len == 1 || sum == 0.0)) {
          new_topic = polyaurn_uniform_topic(u53(o.x, o.y), K);
        } else if (new_topic < 0 || hi32(tt) < 0) {                // UPLDA:1529-1531
          atomicOr(p.status, ST_INVALID_TOPIC);
          new_topic = new_topic < 0 ? 0 : K - 1;
        }
        cnt[new_topic * 64 + lane] += 1;                           // UPLDA:1535
        p.z[beg + t] = new_topic;
        p.zw[ip] = new_topic;
      }
      asm volatile("" ::: "memory");
      w = w1;
#pragma unroll
      for (int m = 0; m < 8; ++m) ra[m] = ran[m];
    }
  }

// cs_kernels_ids.hip.inc — CS_CFG_WIDE_IDS: 64-bit external ids over the 32-bit device ids, and the renumbering of
// the live agents' device ids in place when the device counter nears its limit.  Off the step path.
// Part of the single translation unit crowdstep_hip.hip (included there, in order).
//
// The step kernels read only the ORDER of two ids (right of way, canonical visiting order) and the PARITY of one
// (CS_HLP_ID_PARITY).  After a renumbering at which L agents were alive, the live agent of rank r (ascending id) holds
// device id 2r + parity, and
//   ext(d) = d < dev_base ? ext_of[d >> 1] : ext_base + (d - dev_base)
// with ext_of the ascending external ids of those L agents, dev_base the first device id handed out afterwards (the
// parity of ext_base) and ext_base its external id.  Both order and parity survive, so cell order, in-cell order and
// the kept band windows stay valid.

// external id of device id d (without the flag: no table, dev_base = ext_base = 0, ext(d) = d)
__device__ __forceinline__ uint64_t ext_id_dev(uint32_t d, const uint64_t* __restrict__ tab, uint32_t n_tab,
                                               uint32_t dev_base, uint64_t ext_base) {
  if (d < dev_base && (d >> 1) < n_tab) return tab[d >> 1];
  return ext_base + (uint64_t)(d - dev_base);
}

// The sort: LSD radix over 4-bit digits, a tile of IDS_TILE keys per workgroup (IDS_ITEMS consecutive keys per
// thread, which keeps the scatter stable).  Only the bits below the device counter are sorted.
#define IDS_BLOCK 256u
#define IDS_ITEMS 16u
#define IDS_TILE (IDS_BLOCK * IDS_ITEMS)
#define IDS_RADIX 16u

// the ids of the live slots, compacted in no particular order (one atomic per wave)
__global__ void k_ids_gather(AgentArrays a, uint32_t n, uint32_t* __restrict__ out, uint32_t* __restrict__ count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n && a.cell[i] != CS_INVALID_CELL;
  const unsigned long long m = __ballot(live);
  if (!m) return;
  const int lane = __lane_id();
  const int first = __ffsll((long long)m) - 1;
  uint32_t base = 0;
  if (lane == first) base = atomicAdd(count, (uint32_t)__popcll(m));
  base = __shfl(base, first, 64);
  if (!live) return;
  out[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = a.id[i];
}

// hist[d * n_tiles + t] = keys of tile t whose digit at `shift` is d
__global__ void __launch_bounds__(IDS_BLOCK) k_ids_hist(const uint32_t* __restrict__ keys, uint32_t n, uint32_t shift,
                                                        uint32_t* __restrict__ hist, uint32_t n_tiles) {
  __shared__ uint32_t cnt[IDS_RADIX];
  if (threadIdx.x < IDS_RADIX) cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * IDS_TILE;
  for (uint32_t k = threadIdx.x; k < IDS_TILE; k += IDS_BLOCK)
    if (base + k < n) atomicAdd(&cnt[(keys[base + k] >> shift) & (IDS_RADIX - 1u)], 1u);
  __syncthreads();
  if (threadIdx.x < IDS_RADIX) hist[threadIdx.x * n_tiles + blockIdx.x] = cnt[threadIdx.x];
}

// exclusive scan of the m entries of hist, digit-major, in one workgroup
__global__ void __launch_bounds__(IDS_BLOCK) k_ids_scan(uint32_t* __restrict__ hist, uint32_t m) {
  __shared__ uint32_t s[IDS_BLOCK];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (m + IDS_BLOCK - 1u) / IDS_BLOCK;
  const uint32_t lo = min(m, t * per), hi = min(m, lo + per);
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; ++i) sum += hist[i];
  s[t] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < IDS_BLOCK; d <<= 1) {
    const uint32_t v = t >= d ? s[t - d] : 0u;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  uint32_t run = s[t] - sum;
  for (uint32_t i = lo; i < hi; ++i) {
    const uint32_t v = hist[i];
    hist[i] = run;
    run += v;
  }
}

// stable scatter of one digit: thread t of tile b owns keys [b * IDS_TILE + t * IDS_ITEMS, + IDS_ITEMS)
__global__ void __launch_bounds__(IDS_BLOCK) k_ids_scatter(const uint32_t* __restrict__ keys, uint32_t* __restrict__ out,
                                                           uint32_t n, uint32_t shift, const uint32_t* __restrict__ hist,
                                                           uint32_t n_tiles) {
  __shared__ uint32_t cnt[IDS_RADIX][IDS_BLOCK];  // per digit, per thread: then where its next key of that digit goes
  __shared__ uint32_t seg[IDS_RADIX][IDS_RADIX];
  const uint32_t t = threadIdx.x;
  const uint32_t base = blockIdx.x * IDS_TILE + t * IDS_ITEMS;
  for (uint32_t d = 0; d < IDS_RADIX; ++d) cnt[d][t] = 0;
  for (uint32_t j = 0; j < IDS_ITEMS; ++j)
    if (base + j < n) ++cnt[(keys[base + j] >> shift) & (IDS_RADIX - 1u)][t];
  __syncthreads();
  {  // exclusive scan along the threads for every digit: thread (d, s) takes 16 threads' counts of digit d
    const uint32_t d = t / IDS_RADIX, s = t % IDS_RADIX;
    uint32_t* row = &cnt[d][s * (IDS_BLOCK / IDS_RADIX)];
    uint32_t sum = 0;
    for (uint32_t u = 0; u < IDS_BLOCK / IDS_RADIX; ++u) sum += row[u];
    seg[d][s] = sum;
    __syncthreads();
    uint32_t run = hist[d * n_tiles + blockIdx.x];
    for (uint32_t u = 0; u < s; ++u) run += seg[d][u];
    for (uint32_t u = 0; u < IDS_BLOCK / IDS_RADIX; ++u) {
      const uint32_t v = row[u];
      row[u] = run;
      run += v;
    }
  }
  __syncthreads();
  for (uint32_t j = 0; j < IDS_ITEMS; ++j) {
    if (base + j >= n) break;
    const uint32_t k = keys[base + j];
    out[cnt[(k >> shift) & (IDS_RADIX - 1u)][t]++] = k;
  }
}

// every live agent's new device id: 2 * (its rank among the sorted live ids) + its parity
__global__ void k_ids_renumber(AgentArrays a, uint32_t n, const uint32_t* __restrict__ sorted, uint32_t n_live) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || a.cell[i] == CS_INVALID_CELL) return;
  const uint32_t id = a.id[i];
  uint32_t lo = 0, hi = n_live;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (sorted[mid] < id) lo = mid + 1u;
    else hi = mid;
  }
  a.id[i] = 2u * lo + (id & 1u);
}

// the new table from the old mapping: new_tab[r] = ext(sorted[r])
__global__ void k_ids_table(const uint32_t* __restrict__ sorted, uint32_t n_live, const uint64_t* __restrict__ old_tab,
                            uint32_t old_n, uint32_t dev_base, uint64_t ext_base, uint64_t* __restrict__ new_tab) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n_live) new_tab[r] = ext_id_dev(sorted[r], old_tab, old_n, dev_base, ext_base);
}

// a mesh's renumbering: every live agent's new id from its external id's rank in the mesh-wide table `all` (ascending)
__global__ void k_ids_renumber_ext(AgentArrays a, uint32_t n, const uint64_t* __restrict__ tab, uint32_t n_tab,
                                   uint32_t dev_base, uint64_t ext_base, const uint64_t* __restrict__ all, uint32_t n_all) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || a.cell[i] == CS_INVALID_CELL) return;
  const uint32_t id = a.id[i];
  const uint64_t x = ext_id_dev(id, tab, n_tab, dev_base, ext_base);
  uint32_t lo = 0, hi = n_all;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (all[mid] < x) lo = mid + 1u;
    else hi = mid;
  }
  a.id[i] = 2u * lo + (id & 1u);
}

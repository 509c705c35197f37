// cs_kernel_band_builder.hip.inc -- the body of build_band (cs_kernels_step.hip.inc): the band windows of one band of
// owned rows.  Textually included twice: with its six large arrays as static LDS of the builder kernels (BAND_ARRAY
// declares a __shared__ array), and inside the neighbour kernel's launch (small crowds: the builder workgroups of
// k_step_tiled cut the NEXT step's windows), where the arrays live in the dynamic LDS a window workgroup would use
// (BAND_ARRAY carves them from `band_scratch`: the kernel's static LDS stays what the neighbour pass needs, or a CU would
// hold fewer of its workgroups).  Parameters by the names of build_band's signature.
  // split != 0 (tile engines that overlap the halo exchange with the step): a window with an owned
  // cell within `split` cells of the owned rectangle's edge is a BORDER window.  Border windows are
  // listed from the back of `desc` (desc[desc_cap - 1 - k], k counted in n_blocks[1]) and run as a
  // launch of their own, first; the others from the front (n_blocks[0]) as always.
  __shared__ uint32_t wsum[4];
  __shared__ uint32_t s_carry;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t row0 = g.own_x0 + band * rb;
  const uint32_t nown = min(rb, g.own_x1 - row0);
  const uint32_t ncols = g.own_y1 - g.own_y0;
  // the prefix lives in LDS when the band is narrow enough (binary searches below), else in HBM
  BAND_ARRAY(uint32_t, s_incl, BAND_LDS_COLS)
  uint32_t* __restrict__ incl =
      ncols <= BAND_LDS_COLS ? s_incl : prefix + (unsigned long long)band * ncols;
  auto column_count = [&](uint32_t y) {
    uint32_t c = 0;
    for (uint32_t r = 0; r < nown; ++r) {
      const unsigned long long q = (unsigned long long)(row0 + r) * g.nx + g.own_y0 + y;
      c += cell_start[q + 1] - cell_start[q];
    }
    return c;
  };
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  // What a window STAGES: its columns and h more on either side, of the owned rows and of h ghost
  // rows above and below.  s_all is the inclusive prefix of those per-column counts over the
  // columns [own_y0 - hl, own_y1 + hr) (the owned ones and up to h ghost columns on either side),
  // entry y + hl for owned column y.  A sparse band beside dense rows (the edge of a crowd) stages
  // mostly ghosts: bounding the owned agents alone let such windows overflow the LDS tile, and
  // their 256 agents took the gather path (one such workgroup runs ~100 us).
  BAND_ARRAY(uint32_t, s_all, BAND_LDS_COLS)
  const uint32_t hl = min(h, g.own_y0), hr = min(h, g.nx - g.own_y1);
  const uint32_t ncols_ext = ncols + hl + hr;
  const uint32_t gr0 = row0 > h ? row0 - h : 0u;  // staged rows [gr0, gr1]
  const uint32_t gr1 = min(row0 + nown - 1u + h, g.ncells / g.nx - 1u);
  const bool staged_prefix = ncols_ext <= BAND_LDS_COLS;
  if (ncols <= BAND_LDS_COLS) {
    // the raw counts go to LDS with all loads of the band in flight at once (column = k * 256 +
    // thread: coalesced), then every thread scans BAND_LDS_COLS / 256 consecutive columns
    constexpr uint32_t EPT = BAND_LDS_COLS / 256u;
    uint32_t c[EPT];
    if (staged_prefix) {
#pragma unroll
      for (uint32_t k = 0; k < EPT; ++k) {
        const uint32_t ye = k * 256u + threadIdx.x;  // extended column
        if (ye < ncols_ext) {
          uint32_t cnt = 0;
          for (uint32_t r = gr0; r <= gr1; ++r) {
            const unsigned long long q = (unsigned long long)r * g.nx + (g.own_y0 - hl) + ye;
            cnt += cell_start[q + 1] - cell_start[q];
          }
          s_all[ye] = cnt;
        }
      }
    }
    if (nown == 2u) {  // the usual band: straight-line loads
      uint32_t a0[EPT], a1[EPT], b0[EPT], b1[EPT];
#pragma unroll
      for (uint32_t k = 0; k < EPT; ++k) {
        const uint32_t y = min(k * 256u + threadIdx.x, ncols - 1u);
        const unsigned long long q = (unsigned long long)row0 * g.nx + g.own_y0 + y;
        a0[k] = cell_start[q];
        a1[k] = cell_start[q + 1];
        b0[k] = cell_start[q + g.nx];
        b1[k] = cell_start[q + g.nx + 1];
      }
#pragma unroll
      for (uint32_t k = 0; k < EPT; ++k)
        if (k * 256u + threadIdx.x < ncols) s_incl[k * 256u + threadIdx.x] = (a1[k] - a0[k]) + (b1[k] - b0[k]);
    } else {
#pragma unroll
      for (uint32_t k = 0; k < EPT; ++k) {
        const uint32_t y = k * 256u + threadIdx.x;
        if (y < ncols) s_incl[y] = column_count(y);
      }
    }
    __syncthreads();
    uint32_t ca[EPT];
#pragma unroll
    for (uint32_t k = 0; k < EPT; ++k) {
      const uint32_t y = threadIdx.x * EPT + k;
      c[k] = y < ncols ? s_incl[y] : 0u;
      ca[k] = (staged_prefix && y < ncols_ext) ? s_all[y] : 0u;
    }
    __syncthreads();
    uint32_t mine = 0, mine_a = 0;
#pragma unroll
    for (uint32_t k = 0; k < EPT; ++k) {
      mine += c[k];
      mine_a += ca[k];
    }
    __shared__ uint32_t wsum_a[4];
    const uint32_t w = wave_incl_scan(mine, lane), wa = wave_incl_scan(mine_a, lane);
    if (lane == 63) {
      wsum[wave] = w;
      wsum_a[wave] = wa;
    }
    __syncthreads();
    uint32_t run = w - mine, run_a = wa - mine_a;
    for (int k = 0; k < wave; ++k) {
      run += wsum[k];
      run_a += wsum_a[k];
    }
#pragma unroll
    for (uint32_t k = 0; k < EPT; ++k) {
      const uint32_t y = threadIdx.x * EPT + k;
      run += c[k];
      run_a += ca[k];
      if (y < ncols) s_incl[y] = run;
      if (staged_prefix && y < ncols_ext) s_all[y] = run_a;
    }
    if (threadIdx.x == blockDim.x - 1) s_carry = run;
    __syncthreads();
  } else {
    for (uint32_t base = 0; base < ncols; base += blockDim.x) {
      const uint32_t y = base + threadIdx.x;
      const uint32_t c = y < ncols ? column_count(y) : 0u;
      const uint32_t w = wave_incl_scan(c, lane);
      if (lane == 63) wsum[wave] = w;
      __syncthreads();
      uint32_t woff = 0;
      for (int k = 0; k < wave; ++k) woff += wsum[k];
      if (y < ncols) incl[y] = s_carry + woff + w;
      __syncthreads();
      if (threadIdx.x == blockDim.x - 1) s_carry += woff + w;
      __syncthreads();
    }
  }
  const uint32_t total = s_carry;
  if (threadIdx.x == 0) {
    if (total) atomicAdd(&ctr->n_owned, total);
  }
  // smallest y with incl[y] >= v (ncols if none); incl is non-decreasing
  auto lb = [&](uint32_t v) {
    uint32_t lo = 0, hi = ncols;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (incl[mid] >= v) hi = mid; else lo = mid + 1;
    }
    return lo;
  };
  const bool band_border = split && (row0 < g.own_x0 + split || row0 + nown + split > g.own_x1);
  auto is_border = [&](uint32_t y0, uint32_t y1) {  // y0, y1: columns relative to own_y0
    return split && (band_border || y0 < split || y1 + split >= ncols);
  };
  const uint32_t list_cap = split ? desc_cap / 2u : desc_cap;  // the two lists share the array
  // k: index within its list
  auto emit = [&](uint32_t k, bool border, uint32_t y0, uint32_t y1) {
    if (k >= list_cap) atomicAdd(&ctr->n_win_dropped, 1u);  // (never, if the host's bound holds)
    if (k < list_cap) {
      k = border ? desc_cap - 1u - k : k;
      BlockDesc d;
      d.row0 = row0;
      d.nrows = (unsigned short)nown;
      d.cut = 0;
      d.y0 = g.own_y0 + y0;
      d.y1 = g.own_y0 + y1;
      d.first = 0;
      d.count = 0;
      d.first1 = 0;
      d.count1 = 0;
      desc[k] = d;
    }
  };
  if (ncols <= BAND_LDS_COLS) {
    // Greedy windows: each takes as many whole columns as fit `target` agents (at least one
    // column), so a workgroup of the step kernel is as full as the column sizes allow.  Every
    // non-empty column computes, in parallel, where a window starting there would end and where
    // the next one would start; one thread then follows the chain from the first column.  The
    // searches are chains of dependent LDS reads: a thread runs those of its (up to NQ) columns
    // side by side, branch-free, over a fixed number of halvings.  (s_incl by name: through the
    // `incl` pointer these would be flat loads, several times the latency of a ds_read.)
    BAND_ARRAY(unsigned short, s_end, BAND_LDS_COLS)
    BAND_ARRAY(unsigned short, s_next, BAND_LDS_COLS)
    BAND_ARRAY(unsigned short, s_win, BAND_LDS_COLS)
    BAND_ARRAY(unsigned short, s_cls, BAND_LDS_COLS)  // index of window w within its list | 0x8000 (border)
    __shared__ uint32_t s_nw, s_first, s_first_b, s_y0;
    // Plain windows (cover == 0: cut for this step alone) of bands of one or two rows are cut at AGENT granularity.  The
    // band's agents in the order (column, row, slot) are dealt out `target` at a time: window k owns the positions
    // [k * target, (k + 1) * target) of that order, the band's last window the remainder, so every workgroup of the step
    // kernel but one per band is full.  A run of that order is whole columns, then whole cells of the boundary column,
    // then single agents of one cell, and is therefore one run of slots in each row (BlockDesc::cut).  Every window is
    // found on its own, by two searches in the prefix; no chain.  The existing bounds hold: a band in which some such
    // window would stage more than stage_cap agents or span more than max_cols columns (a sparse band beside dense
    // rows, a crowd's thin edge) is cut by the greedy rule below as before, whole columns per window.  Windows kept
    // for several steps (cover != 0) must own cells, not slots, and are cut below as well.
    const uint32_t n_cut = (total + target - 1u) / max(target, 1u);
    // (a target beyond a workgroup's lanes, CS_TILE_TARGET: windows walked in chunks, cut below as well)
    if (!cover && nown <= 2u && staged_prefix && target != 0u && target <= (uint32_t)TILE_THREADS && total != 0u &&
        n_cut <= BAND_LDS_COLS) {
      __shared__ uint32_t s_cut_bad;
      if (threadIdx.x == 0) s_cut_bad = 0u;
      __syncthreads();
      // smallest column with s_incl[y] >= v (ncols if none)
      auto lb_lds = [&](uint32_t v) {
        uint32_t lo = 0, hi = ncols;
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (s_incl[mid] >= v) hi = mid; else lo = mid + 1;
        }
        return lo;
      };
      for (uint32_t k = threadIdx.x; k < n_cut; k += blockDim.x) {
        const uint32_t p0 = k * target, p1 = min(p0 + target, total);
        const uint32_t ya = lb_lds(p0 + 1u), yb = lb_lds(p1);  // columns of the first and the last owned agent (< ncols)
        // what it would stage: the extended columns [ya + hl - h, yb + hl + h], clipped to the prefix
        const uint32_t yl = ya + hl > h ? ya + hl - h : 0u;
        const uint32_t yr = min(yb + hl + h, ncols_ext - 1u);
        const uint32_t staged = s_all[yr] - (yl == 0u ? 0u : s_all[yl - 1u]);
        if (staged > stage_cap || yb - ya + 1u > max_cols) s_cut_bad = 1u;
        s_win[k] = (unsigned short)ya;
        s_end[k] = (unsigned short)yb;
      }
      __syncthreads();
      if (s_cut_bad == 0u) {  // (block-uniform)
        if (threadIdx.x == 0) {
          uint32_t nb = 0;
          if (split)
            for (uint32_t w = 0; w < n_cut; ++w) {
              const bool b = is_border(s_win[w], s_end[w]);
              s_cls[w] = (unsigned short)(b ? (nb | 0x8000u) : (w - nb));
              nb += b ? 1u : 0u;
            }
          s_first = n_cut - nb ? atomicAdd(&n_blocks[0], n_cut - nb) : 0u;
          s_first_b = nb ? atomicAdd(&n_blocks[1], nb) : 0u;
        }
        __syncthreads();
        // slots of row r in front of band position p, which lies in column y (p == total: y == ncols, the row's end)
        auto row_slot = [&](uint32_t r, uint32_t p, uint32_t y) {
          const unsigned long long q = (unsigned long long)(row0 + r) * g.nx + g.own_y0 + y;
          const uint32_t at = cell_start[q];
          if (y >= ncols) return at;
          const uint32_t in_col = p - (y == 0u ? 0u : s_incl[y - 1u]);  // positions of column y in front of p
          if (nown == 1u) return at + in_col;
          const uint32_t c0 = cell_start[q - (unsigned long long)r * g.nx + 1u] - cell_start[q - (unsigned long long)r * g.nx];
          return r == 0u ? at + min(in_col, c0) : at + (in_col > c0 ? in_col - c0 : 0u);
        };
        for (uint32_t k = threadIdx.x; k < n_cut; k += blockDim.x) {
          const uint32_t p0 = k * target, p1 = min(p0 + target, total);
          const uint32_t ya = s_win[k], yb = s_end[k];
          const uint32_t ye = p1 < total ? lb_lds(p1 + 1u) : ncols;  // column of the first agent behind the window
          const bool b = split && (s_cls[k] & 0x8000u) != 0u;
          uint32_t idx = (b ? s_first_b : s_first) + (split ? (s_cls[k] & 0x7FFFu) : k);
          if (idx >= list_cap) atomicAdd(&ctr->n_win_dropped, 1u);  // (never, if the host's bound holds)
          if (idx < list_cap) {
            idx = b ? desc_cap - 1u - idx : idx;
            BlockDesc d;
            d.row0 = row0;
            d.nrows = (unsigned short)nown;
            d.cut = 1;
            d.y0 = g.own_y0 + ya;
            d.y1 = g.own_y0 + yb;
            d.first = row_slot(0u, p0, ya);
            d.count = row_slot(0u, p1, ye) - d.first;
            d.first1 = nown > 1u ? row_slot(1u, p0, ya) : 0u;
            d.count1 = nown > 1u ? row_slot(1u, p1, ye) - d.first1 : 0u;
            desc[idx] = d;
          }
        }
        return;
      }
    }
    if (threadIdx.x == 0) s_y0 = ncols;  // first non-empty column, found by its own thread below
    __syncthreads();
    constexpr int NQ = 4;
    int halvings = 1;
    while ((1u << halvings) <= ncols_ext) ++halvings;  // 2^halvings > ncols_ext: enough for [0, ncols_ext]
    // the second half of the queries searches s_all (over the extended columns) when STAGED
    auto lb_many = [&](const uint32_t (&v)[2 * NQ], uint32_t (&out)[2 * NQ], auto staged_tag) {
      constexpr bool STAGED = decltype(staged_tag)::value;
      uint32_t lo[2 * NQ], hi[2 * NQ];
#pragma unroll
      for (int k = 0; k < 2 * NQ; ++k) {
        lo[k] = 0;
        hi[k] = (STAGED && k >= NQ) ? ncols_ext : ncols;
      }
      for (int it = 0; it < halvings; ++it) {
        uint32_t mid[2 * NQ], x[2 * NQ];
#pragma unroll
        for (int k = 0; k < 2 * NQ; ++k) {  // the reads first, then the updates
          mid[k] = (lo[k] + hi[k]) >> 1;
          if (STAGED && k >= NQ) x[k] = s_all[min(mid[k], ncols_ext - 1u)];
          else x[k] = s_incl[min(mid[k], ncols - 1u)];
        }
#pragma unroll
        for (int k = 0; k < 2 * NQ; ++k) {
          const bool open = lo[k] < hi[k], ge = x[k] >= v[k];
          hi[k] = (open && ge) ? mid[k] : hi[k];
          lo[k] = (open && !ge) ? mid[k] + 1u : lo[k];
        }
      }
#pragma unroll
      for (int k = 0; k < 2 * NQ; ++k) out[k] = lo[k];
    };
    const uint32_t own_share = (uint32_t)(((unsigned long long)stage_cap * nown) / (nown + 2u * h));
    for (uint32_t base = 0; base < ncols; base += NQ * blockDim.x) {
      uint32_t y[NQ], e_prev[NQ], vab[2 * NQ], yab[2 * NQ];
      bool live[NQ];
#pragma unroll
      for (int k = 0; k < NQ; ++k) {
        y[k] = base + k * blockDim.x + threadIdx.x;
        const uint32_t yy = min(y[k], ncols - 1u);
        e_prev[k] = yy == 0 ? 0u : s_incl[yy - 1];
        live[k] = y[k] < ncols && s_incl[yy] != e_prev[k];  // empty column: no window starts here
        vab[k] = e_prev[k] + target + 1u;
        // the staged tile (h more columns on either side, h ghost rows above and below) must fit
        // the LDS slots of the step kernel, or the whole window takes the gather path
        if (staged_prefix) {
          const uint32_t yl = yy + hl > h ? yy + hl - h : 0u;  // left halo edge, extended column
          vab[NQ + k] = (yl == 0u ? 0u : s_all[yl - 1u]) + stage_cap + 1u;
        } else {  // (a band too wide for the second prefix: ghost rows taken to be as full as the owned ones)
          const uint32_t yl = yy > h ? yy - h : 0u;
          vab[NQ + k] = (yl == 0u ? 0u : s_incl[yl - 1u]) + own_share + 1u;
        }
      }
      // columns < yab[k] keep the window within `target`; columns < yab[NQ + k] (as right halo
      // edge) fit the staging area
      if (staged_prefix) lb_many(vab, yab, std::true_type{});
      else lb_many(vab, yab, std::false_type{});
      uint32_t y1[NQ], vcd[2 * NQ], ycd[2 * NQ];
#pragma unroll
      for (int k = 0; k < NQ; ++k) {
        y1[k] = yab[k] > y[k] ? yab[k] - 1u : y[k];
        uint32_t ys = yab[NQ + k];
        // last owned column = right halo edge - h; if the rest of the band fits there is no
        // bound (the halo ends at the grid's edge)
        if (staged_prefix) ys = ys >= ncols_ext ? ncols - 1u : (ys > h + hl ? ys - 1u - h - hl : 0u);
        else ys = ys >= ncols ? ncols - 1u : (ys > h ? ys - 1u - h : 0u);
        y1[k] = min(max(min(y1[k], ys), y[k]), ncols - 1u);
        // the step kernel's window-relative fixed-point positions span a bounded number of columns
        y1[k] = min(y1[k], y[k] + max_cols - 1u);
        vcd[k] = s_incl[y1[k]];       // -> last non-empty column of the window
        vcd[NQ + k] = vcd[k] + 1u;    // -> next non-empty column, or ncols
      }
      lb_many(vcd, ycd, std::false_type{});
#pragma unroll
      for (int k = 0; k < NQ; ++k)
        if (live[k]) {
          s_end[y[k]] = (unsigned short)max(ycd[k], y[k]);
          s_next[y[k]] = (unsigned short)ycd[NQ + k];
          if (e_prev[k] == 0u) s_y0 = y[k];  // nobody before it: the chain starts here
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      // Two consecutive windows cut by `target` hold more than `target` agents together, so a
      // band has at most `budget` of them; windows cut by the staging bound can be smaller, and
      // where those would break the budget the last window takes the rest of the band (the step
      // kernel walks it in chunks, through its gather path where it does not fit the LDS).
      // (... or their staged agents more than stage_cap together: s_all's total bounds those)
      const uint32_t budget = 2u * (total / target) + 1u + ncols / max_cols +
                              (staged_prefix ? 2u * (s_all[ncols_ext - 1u] / max(stage_cap, 1u)) + 1u : 0u);
      uint32_t nw = 0;
      for (uint32_t y = s_y0; y < ncols; y = s_next[y]) {
        s_win[nw++] = (unsigned short)y;
        if (nw == budget) {
          s_end[y] = (unsigned short)lb(total);  // the band's last non-empty column
          break;
        }
      }
      // The final list, first column | last column << 16, in s_incl (the owned prefix is not needed any more; s_all, the
      // staged prefix, still is).
      // cover != 0 (the engine will step SEVERAL times on these windows: cs_engine, "windows kept"): every column of the
      // band that no window owns, before the first, between two and behind the last, gets a FILLER window of its own,
      // so that the windows tile the band's owned cells completely and an agent that walks, or is added, into a column
      // that is empty now finds a workgroup that steps it.  A filler is cut like a window: by the columns the fixed-point
      // range holds and by what it would STAGE (its own rows are empty, the ghost rows beside them may be the crowd's
      // front: a filler that staged more than the LDS tile holds would send the first agents that walk in down the
      // gather path).  A filler whose cells are empty costs a workgroup that stages its ghosts and leaves.
      uint32_t nf = 0;
      uint32_t* __restrict__ s_final = s_incl;
      if (cover) {
        // smallest extended column whose staged prefix reaches v (ncols_ext if none)
        auto lb_all = [&](uint32_t v) {
          uint32_t lo = 0, hi = ncols_ext;
          while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_all[mid] >= v) hi = mid; else lo = mid + 1;
          }
          return lo;
        };
        uint32_t next_free = 0;  // first column not covered yet
        auto fill = [&](uint32_t a0, uint32_t b0) {  // [a0, b0]
          uint32_t a = a0;
          while (a <= b0 && nf < BAND_LDS_COLS) {
            uint32_t e = min(b0, a + max_cols - 1u);
            if (staged_prefix) {  // (the window builder's own rule for the staging bound, see above)
              const uint32_t yl = a + hl > h ? a + hl - h : 0u;
              // (half the bound: a filler's own cells are empty NOW; what walks in, and the ghost rows filling up
              // beside it, must still fit a step later)
              const uint32_t ys = lb_all((yl == 0u ? 0u : s_all[yl - 1u]) + stage_cap / 2u + 1u);
              const uint32_t last = ys >= ncols_ext ? ncols - 1u : (ys > h + hl ? ys - 1u - h - hl : 0u);
              e = min(e, max(last, a));
            }
            s_final[nf++] = a | (e << 16);
            a = e + 1u;
          }
        };
        // (the windows are read from s_win / s_end, which this does not touch)
        for (uint32_t w = 0; w < nw; ++w) {
          const uint32_t a = s_win[w], e = s_end[a];
          if (a > next_free) fill(next_free, a - 1u);
          if (nf < BAND_LDS_COLS) s_final[nf++] = a | (e << 16);
          next_free = e + 1u;
        }
        if (next_free < ncols) fill(next_free, ncols - 1u);
      } else {
        for (uint32_t w = 0; w < nw; ++w) s_final[nf++] = (uint32_t)s_win[w] | ((uint32_t)s_end[s_win[w]] << 16);
      }
      uint32_t nb = 0;
      for (uint32_t w = 0; w < nf; ++w) {
        const bool b = is_border(s_final[w] & 0xFFFFu, s_final[w] >> 16);
        s_cls[w] = (unsigned short)(b ? (nb | 0x8000u) : (w - nb));
        nb += b ? 1u : 0u;
      }
      s_nw = nf;
      s_first = nf - nb ? atomicAdd(&n_blocks[0], nf - nb) : 0u;
      s_first_b = nb ? atomicAdd(&n_blocks[1], nb) : 0u;
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < s_nw; w += blockDim.x) {
      const bool b = (s_cls[w] & 0x8000u) != 0u;
      emit((b ? s_first_b : s_first) + (s_cls[w] & 0x7FFFu), b, s_incl[w] & 0xFFFFu, s_incl[w] >> 16);
    }
    return;
  }
  // very wide bands (prefix in HBM): windows at fixed quantiles of the band's agent count (a window
  // wider than max_cols columns takes the step kernel's gather path)
  const uint32_t quant = target - target / 8u;
  const uint32_t nw = (total + quant - 1u) / quant;
  for (uint32_t w = threadIdx.x; w < nw; w += blockDim.x) {
    const uint32_t lo = w * quant, hi = lo + quant;
    // first column whose first agent has band index >= lo (excl(y) = incl[y-1])
    const uint32_t a = lo == 0 ? 0u : lb(lo) + 1u;
    if (a >= ncols) continue;
    const uint32_t ea = a == 0 ? 0u : incl[a - 1];
    const uint32_t y0 = lb(ea + 1u);  // skip empty columns
    if (y0 >= ncols) continue;
    const uint32_t e0 = y0 == 0 ? 0u : incl[y0 - 1];
    if (e0 >= hi) continue;  // a single column jumped over this window
    // last column whose first agent has band index < hi
    const uint32_t b = lb(hi);  // columns > b have excl >= hi
    const uint32_t ylast = min(b, ncols - 1u);
    const uint32_t y1 = lb(incl[ylast]);  // drop trailing empty columns
    const bool brd = is_border(y0, y1);
    emit(atomicAdd(&n_blocks[brd ? 1 : 0], 1u), brd, y0, y1);
  }

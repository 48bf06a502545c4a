// kmer_unitigs.hip -- the unitigs of the de Bruijn graph that ONE sorted snapshot implies (tabunitig): which canonical
// k-mers follow which, the maximal non-branching chains of that graph spelled as sequences, and where every key lies in
// them.  Semantics: include/classpro_amd.h, "Unitigs of sorted k-mers"; design: DESIGN.md 9.19.  Included by capi.hip after
// kmer_hetpairs.hip (kl_view, kl_find_group, hp_rule, hp_revcomp, so_scan, ks_keep_count_kernel, ks_alloc, ks_block_scan,
// the scan kernels of kmer_sort.hip, kc_wave_add, set_err and HIPCHK are in scope).  The operand is only read.
//   state    entry i has the states 2i (spells the key X) and 2i+1 (spells rc(X)); flip(s) = s ^ 1.  A state is below 2^31.
//   adj      one lane per entry.  rc(X) once; the successor c of a string w with reverse complement r is
//            f = (w << 2 | c) under the 2K-bit mask, and its reverse complement is r >> 2 | (3-c) << 2K-2, so the canonical
//            form is one compare and no further reversal.  Eight look-ups by kl_find_group, one after the other; a
//            neighbour counts when it is found and its count lies in the range.  All of it is arithmetic on kt_u128.
//   link     one lane per entry, both states.  A state whose nibble has one bit finds that neighbour again, reads its
//            byte and applies the four conditions.  The lane of s that finds s -> t stores prev[flip(s)] = flip(t): that
//            is the mirror link flip(t) -> flip(s), so both prev of an entry are stored by the entry's own lane, together
//            with the two ranking words.  prev is -1 for no link in and -2 for a state of an entry that is not in.
//   rank     pointer jumping IN PLACE over one 64-bit word per state: bit 63 resolved, bits 31..61 the distance, bits 0..30
//            a state.  An unresolved word says "that state lies so many links before me"; a resolved one names the head.
//            A jump is one 8-byte load of the pointed word and one 8-byte store of the own.  Whatever mixture of old and
//            new words a round reads, every word stays true, so the end state does not depend on scheduling: only the
//            number of rounds does (at most the double-buffered ceil(log2) + 1).  The load of another lane's word and
//            the store of the own are relaxed atomics of agent scope: never torn, and a stale copy would be an old, true
//            word (system and workgroup scope measured the same: DESIGN.md 9.19).  A round that resolves nothing ends it:
//            the unresolved state nearest its head would have been resolved.  What is left lies on closed chains, whose
//            distances are clamped at 2^31-1 and mean nothing.
//   closed   the unresolved states and their prev go to the host as a compacted list (an atomic cursor; the host sorts).
//            The host walks every closed chain from its smallest state, which is always a forward state 2i, numbers it,
//            marks its mirror image dead and sends the words back.  Right at any size; serial in the chain's length.
//   choose   one lane per state.  A tail (no link out: prev[flip(s)] = -1) with head h and distance d keeps the chain iff
//            h < flip(s); it then stores d into the head's word and the head's orientation into the entry's head byte.  A
//            node has at most one kept head, so heads are numbered per ENTRY: members per tile, so_scan, ranks in the tile.
//   number   a block per tile of KS_TILE entries: ordinal of every kept head, its length into off[u+1], its flag.
//   spell    one lane per state of a kept chain: its last base at off[u]+K-1+d, the head also its first K-1 bases, the
//            count into kc[u] by a 64-bit atomic, d_utg and d_at.
// All sums are integer atomics: nothing depends on grid, block size or scheduling.
#include <algorithm>
#include <functional>
#include <new>

#define UG_RES    (1ull << 63)             // a ranking word: resolved -- the state in bits 0..30 is the head
#define UG_DEAD   (1ull << 62)             // ... a state of an entry that is not in, or of a dropped closed chain
#define UG_PMASK  0x7fffffffull
#define UG_DMAX   0x7fffffffull
#define UG_MAX_N  ((int64_t)1 << 30)       // entries at most when unitigs are wanted
#define UG_ROUNDS 64                       // jump rounds at most: 32 suffice for 2^31 states
#define UG_PER_LANE (KS_TILE/KS_BLOCK)
#define UG_HEAD   3u                       // a head byte: 1 the kept head is 2i, 2 it is 2i+1
#define UG_CIRC   4u                       // ... and its chain is closed
enum { UG_OPEN = 11, UG_NCYC = 12, UG_CIRCS = 13, UG_ROUND0 = 16, UG_CTL = UG_ROUND0+UG_ROUNDS };    // words of the control block

struct cp_unitigs
  { int K;
    int64_t count, bases;
    char *seq;                             // bases (null without sequences or when empty)
    int64_t *off, *kc;                     // count+1 and count
    uint8_t *flag;                         // count
  };

// the successor c of the string w whose reverse complement is r: its canonical form; *fwd = the string is that form
__device__ static inline kt_u128 ug_succ(kt_u128 w, kt_u128 r, int K, int c, bool *fwd, bool *pal)
{ const kt_u128 f = ((w << 2) & ((((kt_u128)1) << (2*K))-1)) | (kt_u128)c;
  const kt_u128 b = (r >> 2) | (((kt_u128)(3-c)) << (2*K-2));
  *fwd = f <= b;
  *pal = f == b;
  return f < b ? f : b;
}

// the ordinal of the key y when it is found and in, otherwise -1
template <bool LO_ONLY>
__device__ static inline int64_t ug_find(const kl_view &t, kt_u128 y, hp_rule r)
{ const unsigned long long qh[1] = { (unsigned long long)(y >> 63) }, ql[1] = { (unsigned long long)y & KT_M63 };
  int64_t pos[1];
  kl_find_group<LO_ONLY,KL_INTERP != 0,1>(t,qh,ql,1,pos);
  if (pos[0] < 0) return -1;
  const int64_t at = min(max(pos[0],(int64_t)0),t.n-1);
  const unsigned long long cy = t.cnt[at];
  return cy >= r.cmin && cy <= r.cmax ? at : -1;
}

__device__ static inline kt_u128 ug_key(const kl_view &t, bool with_hi, int64_t i)
{ return (((kt_u128)(with_hi ? t.hi[i] : 0)) << 63) | (kt_u128)t.lo[i]; }

// adj[i] = the adjacency byte of entry i; tally += in keys, isolated keys, tips, branching keys, arcs
template <bool LO_ONLY>
__global__ void __launch_bounds__(KT_BLOCK) ug_adj_kernel(kl_view t, int K, hp_rule r, uint8_t *adj, unsigned long long *tally)
{ unsigned long long nkeys = 0, niso = 0, ntip = 0, nbranch = 0, narc = 0;
  const bool with_hi = 2*K > 63;                           // below that hi[] is zero for every key and is not loaded
  for (int64_t i = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; i < t.n; i += (int64_t)gridDim.x*blockDim.x)
    { const unsigned long long cx = t.cnt[i];
      unsigned int b = 0;
      if (cx >= r.cmin && cx <= r.cmax)
        { const kt_u128 x = ug_key(t,with_hi,i), rc = hp_revcomp(x,K);
          for (int q = 0; q < (x == rc ? 4 : 8); q++)
            { bool fwd, pal;
              const kt_u128 y = ug_succ(q < 4 ? x : rc,q < 4 ? rc : x,K,q & 3,&fwd,&pal);
              if (ug_find<LO_ONLY>(t,y,r) >= 0) b |= 1u << q;
            }
          if (x == rc) b |= b << 4;                        // a palindrome: the two states spell the same string
          const unsigned int f = b & 15u, v = b >> 4;
          nkeys++;
          niso += b == 0;
          ntip += (f == 0) != (v == 0);
          nbranch += __popc(f) >= 2 || __popc(v) >= 2;
          narc += __popc(b);
        }
      adj[i] = (uint8_t)b;
    }
  kc_wave_add(tally+CP_UTG_KEYS,nkeys);
  kc_wave_add(tally+CP_UTG_ISOLATED,niso);
  kc_wave_add(tally+CP_UTG_TIPS,ntip);
  kc_wave_add(tally+CP_UTG_BRANCHING,nbranch);
  kc_wave_add(tally+CP_UTG_ARCS,narc);
}

__device__ static inline unsigned long long ug_word0(int prev, int64_t s)
{ return prev == -2 ? UG_DEAD : prev < 0 ? UG_RES | (unsigned long long)s : (1ull << 31) | (unsigned long long)prev; }

// prev[2i], prev[2i+1] and the two ranking words of every entry i; ctl[UG_OPEN] += the states with a link in
template <bool LO_ONLY>
__global__ void __launch_bounds__(KT_BLOCK) ug_link_kernel(kl_view t, int K, hp_rule r, const uint8_t *adj, int2 *prev,
                                                           ulonglong2 *word, unsigned long long *ctl)
{ unsigned long long nopen = 0;
  const bool with_hi = 2*K > 63;
  for (int64_t i = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; i < t.n; i += (int64_t)gridDim.x*blockDim.x)
    { const unsigned long long cx = t.cnt[i];
      const bool in = cx >= r.cmin && cx <= r.cmax;
      const unsigned int a = adj[i];
      int p[2] = { in ? -1 : -2, in ? -1 : -2 };           // p[o] = prev of the state 2i+o
      if (in && a)
        { const kt_u128 x = ug_key(t,with_hi,i), rc = hp_revcomp(x,K);
          for (int o = 0; o < 2 && x != rc; o++)
            { const unsigned int nib = (a >> (4*o)) & 15u;
              if (__popc(nib) != 1) continue;
              bool fwd, pal;
              const kt_u128 y = ug_succ(o ? rc : x,o ? x : rc,K,__ffs(nib)-1,&fwd,&pal);
              if (pal) continue;
              const int64_t j = ug_find<LO_ONLY>(t,y,r);
              if (j < 0 || j == i) continue;               // the node itself: a homopolymer loop or a hairpin
              const int ot = fwd ? 0 : 1;                  // the successor state is 2j+ot; its flip must have one way out
              if (__popc((adj[j] >> (4*(1-ot))) & 15u) != 1) continue;
              p[1-o] = (int)(2*j+(1-ot));                  // 2i+o -> 2j+ot is flip(2j+ot) -> flip(2i+o)
            }
        }
      prev[i] = make_int2(p[0],p[1]);
      word[i] = make_ulonglong2(ug_word0(p[0],2*i),ug_word0(p[1],2*i+1));
      nopen += (p[0] >= 0)+(p[1] >= 0);
    }
  kc_wave_add(ctl+UG_OPEN,nopen);
}

// one round of jumps over the ns states; *done += the states it resolved
__global__ void __launch_bounds__(KT_BLOCK) ug_jump_kernel(unsigned long long *word, int64_t ns, unsigned long long *done)
{ unsigned long long nres = 0;
  for (int64_t s = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; s < ns; s += (int64_t)gridDim.x*blockDim.x)
    { const unsigned long long w = word[s];                // only this lane stores it
      if (w & (UG_RES | UG_DEAD)) continue;
      const int64_t p = min((int64_t)(w & UG_PMASK),ns-1);
      const unsigned long long v = __hip_atomic_load(word+p,__ATOMIC_RELAXED,__HIP_MEMORY_SCOPE_AGENT);
      const unsigned long long d = min(((w >> 31) & UG_DMAX)+((v >> 31) & UG_DMAX),UG_DMAX);
      __hip_atomic_store(word+s,(v & UG_RES) | (d << 31) | (v & UG_PMASK),__ATOMIC_RELAXED,__HIP_MEMORY_SCOPE_AGENT);
      nres += (v & UG_RES) != 0;
    }
  kc_wave_add(done,nres);
}

// the unresolved states with their prev, state << 32 | prev, in any order; cap of them at most
__global__ void __launch_bounds__(KT_BLOCK) ug_closed_kernel(const unsigned long long *word, const int *prev, int64_t ns,
                                                             unsigned long long *list, unsigned long long cap,
                                                             unsigned long long *cursor)
{ for (int64_t s = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; s < ns; s += (int64_t)gridDim.x*blockDim.x)
    { if (word[s] & (UG_RES | UG_DEAD)) continue;
      const unsigned long long at = atomicAdd(cursor,1ull);
      if (at < cap) list[at] = ((unsigned long long)s << 32) | (unsigned long long)(unsigned int)prev[s];
    }
}

// the words of the closed chains as the host numbered them: m pairs (state, word); a head also gets its head byte
__global__ void __launch_bounds__(KT_BLOCK) ug_reopen_kernel(const unsigned long long *pairs, int64_t m, unsigned long long *word,
                                                             int64_t ns, uint8_t *head)
{ for (int64_t k = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; k < m; k += (int64_t)gridDim.x*blockDim.x)
    { const unsigned long long s = pairs[2*k], w = pairs[2*k+1];
      if ((int64_t)s >= ns) continue;
      word[s] = w;
      if ((w & UG_RES) && (w & UG_PMASK) == s) head[s >> 1] = (uint8_t)((1u+(unsigned int)(s & 1)) | UG_CIRC);
    }
}

// every tail decides for its chain: the kept head's word gets the tail's distance, the entry its head byte
__global__ void __launch_bounds__(KT_BLOCK) ug_choose_kernel(unsigned long long *word, const int *prev, int64_t ns, uint8_t *head)
{ for (int64_t s = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; s < ns; s += (int64_t)gridDim.x*blockDim.x)
    { if (prev[s ^ 1] != -1) continue;                     // a link out, or not in
      const unsigned long long w = word[s];                // a tail's own word: nobody stores it here unless it is its own head
      if (!(w & UG_RES)) continue;
      const int64_t h = min((int64_t)(w & UG_PMASK),ns-1);
      if (h >= (s ^ 1)) continue;                          // the mirror image starts lower: it is the one that is spelled
      word[h] = UG_RES | (w & (UG_DMAX << 31)) | (unsigned long long)h;
      head[h >> 1] = (uint8_t)(1u+(unsigned int)(h & 1));
    }
}

// the predicate of ks_keep_count_kernel: entry i has a kept head
struct ug_is_head
  { const uint8_t *head;
    __device__ bool operator()(int64_t i) const { return head[i] != 0; }
  };

// tile_n holds the inclusive sums.  Kept head of entry i: ord[i] = its unitig u, off[u+1] = its bases, flag[u]; the
// longest and the closed ones into the tally
__global__ void __launch_bounds__(KS_BLOCK) ug_number_kernel(const uint8_t *head, const unsigned long long *word, int64_t n,
                                                             int K, const int64_t *tile_n, int64_t count, int64_t *ord,
                                                             int64_t *off, uint8_t *flag, unsigned long long *tally)
{ __shared__ unsigned long long part[KS_BLOCK];
  const int64_t t = blockIdx.x, i0 = t*KS_TILE+(int64_t)threadIdx.x*UG_PER_LANE;
  unsigned int mine = 0;
  for (int k = 0; k < UG_PER_LANE; k++)
    if (i0+k < n) mine += head[i0+k] != 0;
  int64_t u = (t ? tile_n[t-1] : 0)+(int64_t)(ks_block_scan((unsigned long long)mine,part)-(unsigned long long)mine);
  unsigned long long longest = 0, ncirc = 0;
  for (int k = 0; k < UG_PER_LANE; k++)
    { if (i0+k >= n) break;
      const unsigned int hb = head[i0+k];
      if (!hb || u >= count) continue;
      const int64_t h = 2*(i0+k)+(int64_t)(hb & UG_HEAD)-1;
      const unsigned long long len = ((word[h] >> 31) & UG_DMAX)+(unsigned long long)K;     // nodes + K - 1
      ord[i0+k] = u;
      off[u+1] = (int64_t)len;
      flag[u] = (uint8_t)((hb & UG_CIRC) ? 1 : 0);
      longest = max(longest,len);
      ncirc += (hb & UG_CIRC) != 0;
      u++;
    }
  for (int w = warpSize/2; w > 0; w >>= 1) longest = max(longest,(unsigned long long)__shfl_down(longest,w));
  if ((threadIdx.x & (warpSize-1)) == 0 && longest) atomicMax(tally+CP_UTG_LONGEST,longest);
  kc_wave_add(tally+UG_CIRCS,ncirc);
}

// every state of a kept chain: its base, its count, where it lies
__global__ void __launch_bounds__(KT_BLOCK) ug_spell_kernel(kl_view t, int K, const unsigned long long *word, const uint8_t *head,
                                                            const int64_t *ord, const int64_t *off, int64_t count, int64_t bases,
                                                            char *seq, unsigned long long *kc, int64_t *utg, int64_t *at)
{ const bool with_hi = 2*K > 63;
  const int64_t ns = 2*t.n;
  for (int64_t s = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; s < ns; s += (int64_t)gridDim.x*blockDim.x)
    { const unsigned long long w = word[s];
      if (!(w & UG_RES)) continue;
      const int64_t h = min((int64_t)(w & UG_PMASK),ns-1), i = s >> 1;
      if ((head[h >> 1] & UG_HEAD) != 1u+(unsigned int)(h & 1)) continue;
      const int64_t u = ord[h >> 1], d = h == s ? 0 : (int64_t)((w >> 31) & UG_DMAX);
      if (u < 0 || u >= count) continue;
      if (seq)
        { const kt_u128 x = ug_key(t,with_hi,i), str = (s & 1) ? hp_revcomp(x,K) : x;
          const int64_t base = off[u], pos = base+K-1+d;
          if (pos < bases) seq[pos] = "ACGT"[(int)((unsigned long long)str & 3)];
          if (h == s)
            for (int k = 0; k < K-1 && base+k < bases; k++) seq[base+k] = "ACGT"[(int)((unsigned long long)(str >> (2*(K-1-k))) & 3)];
        }
      if (kc) atomicAdd(kc+u,t.cnt[i]);
      if (utg) utg[i] = u;
      if (at) at[i] = 2*d+(s & 1);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

// v[0..n) to its inclusive scan for any n below 2^36: the chunk sums are scanned by so_scan.  `first` is room for
// (n + KS_CHUNK - 1) / KS_CHUNK + 1 words, `second` what so_scan needs for that many
static int ug_scan(int64_t *v, int64_t n, unsigned long long *first, unsigned long long *second, hipStream_t st)
{ const int64_t nchunk = (n+KS_CHUNK-1)/KS_CHUNK;
  HIPCHK(hipMemsetAsync(first,0,8,st));
  ks_chunk_sum_kernel<<<(unsigned)nchunk,KS_BLOCK,0,st>>>(v,n,first+1);
  so_scan((int64_t *)first+1,nchunk,second,st);            // first[b] = the sum of the chunks before b
  ks_chunk_scan_kernel<<<(unsigned)nchunk,KS_BLOCK,0,st>>>(v,n,first);
  HIPCHK(hipGetLastError());
  return CP_OK;
}

// The closed chains on the host: `list` holds state << 32 | prev of every state on one.  Returns the (state, word) pairs.
static int ug_close_chains(const char *who, std::vector<unsigned long long> &list, std::vector<unsigned long long> &pairs)
{ std::sort(list.begin(),list.end());
  const size_t m = list.size();
  auto find = [&](unsigned long long s) -> size_t
    { const size_t k = (size_t)(std::lower_bound(list.begin(),list.end(),s << 32)-list.begin());
      return k < m && (list[k] >> 32) == s ? k : m;
    };
  std::vector<uint8_t> seen(m,0);
  pairs.clear();
  pairs.reserve(2*m);
  for (size_t k0 = 0; k0 < m; k0++)
    { if (seen[k0]) continue;
      const unsigned long long s0 = list[k0] >> 32;        // the smallest state of the chain and of its mirror image
      if (s0 & 1) return set_err(CP_EHIP,std::string(who)+": internal: a closed chain that starts at a reverse state");
      const size_t first = pairs.size();
      unsigned long long s = s0, d = 0;
      do
        { const size_t k = find(s), f = find(s ^ 1);
          if (k == m || f == m || seen[k] || seen[f] || d >= m)
            return set_err(CP_EHIP,std::string(who)+": internal: a closed chain that does not close");
          seen[k] = seen[f] = 1;
          pairs.push_back(s);
          pairs.push_back(UG_RES | (d << 31) | s0);
          pairs.push_back(s ^ 1);
          pairs.push_back(UG_DEAD);
          d++;
          s = (list[f] & 0xffffffffull) ^ 1;               // next(s) = flip(prev(flip(s)))
        }
      while (s != s0);
      pairs[first+1] = UG_RES | ((d-1) << 31) | s0;        // the head's word carries the last distance
    }
  return CP_OK;
}

// the passes; scratch and the result's memory are freed by the caller when this fails
static int ug_run(const cp_kmer_sorted *s, hp_rule r, bool chains, bool spell, int64_t *tally, uint8_t *d_adj, int64_t *d_utg,
                  int64_t *d_at, hipStream_t st, cp_unitigs *res, void **scratch, void **extra)
{ const char *who = "cp_kmer_sorted_unitigs";
  const kl_view t = kl_view_of(s);
  const bool lo_only = kl_lo_only(s);
  const int64_t n = s->n, ns = 2*n, ntile = (n+KS_TILE-1)/KS_TILE;
  unsigned long long h_ctl[UG_CTL];
  memset(h_ctl,0,sizeof(h_ctl));
  int64_t rounds = 0, jump_ns = 0;
  if (n > 0)
    { // the control block, then per entry: two words, the ordinal, two prev, the head byte, the adjacency byte
      const int64_t nfirst = (n+KS_CHUNK-1)/KS_CHUNK+2, nsecond = (std::max(nfirst,ntile)+KS_CHUNK-1)/KS_CHUNK+1;
      const size_t words = UG_CTL+(chains ? (size_t)(3*n+ntile+nfirst+nsecond) : 0);
      const size_t bytes = words*8+(chains ? (size_t)n*9 : 0)+(d_adj ? 0 : (size_t)n);
      int rc = ks_alloc(who,scratch,bytes,"the ranking words, the links and the adjacency bytes");
      if (rc != CP_OK) return rc;
      unsigned long long *ctl = (unsigned long long *)*scratch, *word = ctl+UG_CTL;
      int64_t *ord = (int64_t *)(word+2*n), *tile_n = ord+n;
      unsigned long long *first = (unsigned long long *)(tile_n+ntile), *second = first+nfirst;
      int *prev = (int *)(chains ? second+nsecond : word);
      uint8_t *head = (uint8_t *)(chains ? prev+2*n : prev);
      uint8_t *adj = d_adj ? d_adj : chains ? head+n : (uint8_t *)word;
      HIPCHK(hipMemsetAsync(ctl,0,UG_CTL*8,st));
      const int grid = (int)std::min<int64_t>((n+KT_BLOCK-1)/KT_BLOCK,16384);
      const int sgrid = (int)std::min<int64_t>((ns+KT_BLOCK-1)/KT_BLOCK,16384);
      if (lo_only) ug_adj_kernel<true><<<grid,KT_BLOCK,0,st>>>(t,s->K,r,adj,ctl);
      else ug_adj_kernel<false><<<grid,KT_BLOCK,0,st>>>(t,s->K,r,adj,ctl);
      HIPCHK(hipGetLastError());
      if (chains)
        { HIPCHK(hipMemsetAsync(head,0,(size_t)n,st));
          if (lo_only) ug_link_kernel<true><<<grid,KT_BLOCK,0,st>>>(t,s->K,r,adj,(int2 *)prev,(ulonglong2 *)word,ctl);
          else ug_link_kernel<false><<<grid,KT_BLOCK,0,st>>>(t,s->K,r,adj,(int2 *)prev,(ulonglong2 *)word,ctl);
          HIPCHK(hipGetLastError());
          HIPCHK(hipMemcpyAsync(h_ctl,ctl,UG_CTL*8,hipMemcpyDeviceToHost,st));
          HIPCHK(hipStreamSynchronize(st));
          unsigned long long open = h_ctl[UG_OPEN];        // the states that do not know their head yet
          const auto t0 = std::chrono::steady_clock::now();
          while (open > 0 && rounds < UG_ROUNDS)
            { unsigned long long done = 0;
              ug_jump_kernel<<<sgrid,KT_BLOCK,0,st>>>(word,ns,ctl+UG_ROUND0+rounds);
              HIPCHK(hipGetLastError());
              HIPCHK(hipMemcpyAsync(&done,ctl+UG_ROUND0+rounds,8,hipMemcpyDeviceToHost,st));
              HIPCHK(hipStreamSynchronize(st));
              rounds++;
              if (done == 0 || done > open) break;
              open -= done;
            }
          jump_ns = (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now()-t0).count();
          if (open > 0)                                    // closed chains: numbered on the host
            { rc = ks_alloc(who,extra,(size_t)open*32,"the states of the closed chains");
              if (rc != CP_OK) return rc;
              unsigned long long *list = (unsigned long long *)*extra;
              ug_closed_kernel<<<sgrid,KT_BLOCK,0,st>>>(word,prev,ns,list,open,ctl+UG_NCYC);
              HIPCHK(hipGetLastError());
              std::vector<unsigned long long> h_list((size_t)open), pairs;
              unsigned long long got = 0;
              HIPCHK(hipMemcpyAsync(&got,ctl+UG_NCYC,8,hipMemcpyDeviceToHost,st));
              HIPCHK(hipMemcpyAsync(h_list.data(),list,(size_t)open*8,hipMemcpyDeviceToHost,st));
              HIPCHK(hipStreamSynchronize(st));
              if (got != open) return set_err(CP_EHIP,std::string(who)+": internal: the jump rounds and the closed chains disagree");
              rc = ug_close_chains(who,h_list,pairs);
              if (rc != CP_OK) return rc;
              HIPCHK(hipMemcpyAsync(list,pairs.data(),pairs.size()*8,hipMemcpyHostToDevice,st));
              const int64_t m = (int64_t)(pairs.size()/2);
              ug_reopen_kernel<<<(int)std::min<int64_t>((m+KT_BLOCK-1)/KT_BLOCK,16384),KT_BLOCK,0,st>>>(list,m,word,ns,head);
              HIPCHK(hipGetLastError());
              HIPCHK(hipStreamSynchronize(st));            // `pairs` is read until here
            }
          ug_choose_kernel<<<sgrid,KT_BLOCK,0,st>>>(word,prev,ns,head);
          HIPCHK(hipGetLastError());
          ks_keep_count_kernel<<<(unsigned)ntile,KS_BLOCK,0,st>>>(ug_is_head{ head },n,tile_n);
          HIPCHK(hipGetLastError());
          so_scan(tile_n,ntile,second,st);
          HIPCHK(hipGetLastError());
          HIPCHK(hipMemcpyAsync(&res->count,tile_n+ntile-1,8,hipMemcpyDeviceToHost,st));
          HIPCHK(hipStreamSynchronize(st));
          const int64_t count = res->count;
          if (count > 0)
            { rc = ks_alloc(who,(void **)&res->off,(size_t)(count+1)*8,"the offsets of the unitigs");
              if (rc == CP_OK) rc = ks_alloc(who,(void **)&res->kc,(size_t)count*8,"the count sums of the unitigs");
              if (rc == CP_OK) rc = ks_alloc(who,(void **)&res->flag,(size_t)count,"the flags of the unitigs");
              if (rc != CP_OK) return rc;
              HIPCHK(hipMemsetAsync(res->off,0,8,st));
              HIPCHK(hipMemsetAsync(res->kc,0,(size_t)count*8,st));
              ug_number_kernel<<<(unsigned)ntile,KS_BLOCK,0,st>>>(head,word,n,s->K,tile_n,count,ord,res->off,res->flag,ctl);
              HIPCHK(hipGetLastError());
              rc = ug_scan(res->off+1,count,first,second,st);
              if (rc != CP_OK) return rc;
              HIPCHK(hipMemcpyAsync(&res->bases,res->off+count,8,hipMemcpyDeviceToHost,st));
              HIPCHK(hipStreamSynchronize(st));
              if (spell)
                { rc = ks_alloc(who,(void **)&res->seq,(size_t)res->bases,"the sequences of the unitigs");
                  if (rc != CP_OK) return rc;
                }
            }
          if (d_utg) HIPCHK(hipMemsetAsync(d_utg,0xff,(size_t)n*8,st));      // -1 for an entry that is not in
          if (d_at) HIPCHK(hipMemsetAsync(d_at,0xff,(size_t)n*8,st));
          if (count > 0)
            { ug_spell_kernel<<<sgrid,KT_BLOCK,0,st>>>(t,s->K,word,head,ord,res->off,count,res->bases,res->seq,
                                                      (unsigned long long *)res->kc,d_utg,d_at);
              HIPCHK(hipGetLastError());
            }
        }
      HIPCHK(hipMemcpyAsync(h_ctl,ctl,UG_CTL*8,hipMemcpyDeviceToHost,st));
    }
  HIPCHK(hipStreamSynchronize(st));
  if (tally)
    { for (int k = 0; k < CP_UTG_WIDTH; k++) tally[k] = (int64_t)h_ctl[k];
      tally[CP_UTG_UNITIGS] = chains ? res->count : 0;
      tally[CP_UTG_BASES] = chains ? res->bases : 0;
      tally[CP_UTG_CIRCULAR] = (int64_t)h_ctl[UG_CIRCS];
      tally[CP_UTG_ROUNDS] = rounds;
      tally[CP_UTG_JUMP_NS] = jump_ns;
    }
  return CP_OK;
}

static void ug_free(cp_unitigs *u)
{ if (!u) return;
  if (u->seq) (void)hipFree(u->seq);
  if (u->off) (void)hipFree(u->off);
  if (u->kc) (void)hipFree(u->kc);
  if (u->flag) (void)hipFree(u->flag);
  delete u;
}

extern "C" int cp_kmer_sorted_unitigs(const cp_kmer_sorted *s, const int64_t *range, int64_t *tally, uint8_t *d_adj,
                                      int64_t *d_utg, int64_t *d_at, void *stream, cp_unitigs **out)
{ const char *who = "cp_kmer_sorted_unitigs";
  if (out) *out = nullptr;
  if (!s || (!tally && !d_adj && !d_utg && !d_at && !out)) return set_err(CP_EINVAL,std::string(who)+": bad argument");
  if (!s->ready) return set_err(CP_EINVAL,std::string(who)+": the snapshot is still being loaded");
  hp_rule r{ 1, (unsigned long long)INT64_MAX };
  if (range)
    { if (range[0] < 1 || range[1] < range[0]) return set_err(CP_EINVAL,std::string(who)+": a count range needs 1 <= min <= max");
      r.cmin = (unsigned long long)range[0];
      r.cmax = (unsigned long long)range[1];
    }
  const bool chains = out || d_utg || d_at;
  if (chains && s->n > UG_MAX_N) return set_err(CP_EINVAL,std::string(who)+": more than 2^30 entries");
  hipStream_t st = (hipStream_t)stream;
  cp_unitigs *res = new (std::nothrow) cp_unitigs();
  if (!res) return set_err(CP_ENOMEM,std::string(who)+": out of memory");
  res->K = s->K;
  void *scratch = nullptr, *extra = nullptr;
  int rc;
  try { rc = ug_run(s,r,chains,out != nullptr,tally,d_adj,d_utg,d_at,st,res,&scratch,&extra); }
  catch (const std::bad_alloc &) { rc = set_err(CP_ENOMEM,std::string(who)+": out of host memory for the closed chains"); }
  if (rc != CP_OK) (void)hipStreamSynchronize(st);
  if (scratch) (void)hipFree(scratch);
  if (extra) (void)hipFree(extra);
  if (rc != CP_OK || !out)
    { ug_free(res);
      return rc;
    }
  *out = res;
  return CP_OK;
}

extern "C" int64_t cp_unitigs_count(const cp_unitigs *u) { return u ? u->count : 0; }
extern "C" int64_t cp_unitigs_bases(const cp_unitigs *u) { return u ? u->bases : 0; }

extern "C" int cp_unitigs_arrays(const cp_unitigs *u, const char **d_seq, const int64_t **d_off, const int64_t **d_kc,
                                 const uint8_t **d_flag)
{ if (!u) return set_err(CP_EINVAL,"cp_unitigs_arrays: bad argument");
  if (d_seq) *d_seq = u->seq;
  if (d_off) *d_off = u->off;
  if (d_kc) *d_kc = u->kc;
  if (d_flag) *d_flag = u->flag;
  return CP_OK;
}

extern "C" void cp_unitigs_destroy(cp_unitigs *u) { ug_free(u); }

extern "C" int64_t cp_unitig_n50(const int64_t *len, int64_t n)
{ if (n < 0 || (n > 0 && !len)) return set_err(CP_EINVAL,"cp_unitig_n50: bad argument");
  if (n == 0) return 0;
  std::vector<int64_t> v(len,len+n);
  std::sort(v.begin(),v.end(),std::greater<int64_t>());
  unsigned __int128 total = 0, run = 0;
  for (int64_t x : v)
    { if (x < 0) return set_err(CP_EINVAL,"cp_unitig_n50: a negative length");
      total += (unsigned __int128)x;
    }
  for (int64_t x : v)
    { run += (unsigned __int128)x;
      if (2*run >= total) return x;
    }
  return 0;
}

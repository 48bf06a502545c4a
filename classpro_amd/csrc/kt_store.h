// kt_store.h -- the host-side life cycle that the two device k-mer tables share: the label table of kmer_table.hip and
// the count table of kmer_counts.hip.  Allocation and fill, the control-block read-back, growth by rehash, creation and
// destruction, the failure bitmaps and the add driver (launch, read back, grow, replay the failed positions).  Included
// by the two .hip files, which capi.hip includes: set_err, HIPCHK and the library's error contract are in scope.
//
// A table is a kt_store<SLOT, CTL> plus what only it holds.  SLOT is 32 bytes, begins with the key words hi and lo
// (kt_common.h) and keeps its counts in a member cnt, one word or an array of four.  CTL begins with the four counters
// below; the store touches no other word of it.  Messages start with the table's public name (cp_kmer_table,
// cp_kmer_counts).
#pragma once
#include <cstddef>
#include <type_traits>
#include "kt_common.h"

template <class SLOT, class CTL>
struct kt_store
  { static_assert(sizeof(SLOT) == 32, "one 32-byte slot per key");
    static_assert(!std::is_array<decltype(SLOT::cnt)>::value || std::extent<decltype(SLOT::cnt)>::value == 4,
                  "the rehash copies an array payload as four counts");
    static_assert(offsetof(CTL,n_fail) == 0        // failed inserts of the last add / replay launch
                  && offsetof(CTL,n_occ) == 8      // occupied slots = distinct keys
                  && offsetof(CTL,n_skip) == 16    // k-mer positions skipped (a byte other than upper-case A C G T)
                  && offsetof(CTL,n_rfail) == 24,  // failed inserts of the last rehash
                  "both control blocks begin with the same four counters");
    const char *name;                    // prefix of the messages
    int K, device;
    SLOT *tab;
    unsigned long long slots;
    CTL *ctl;                            // device
    CTL *h_ctl;                          // pinned host copy
    unsigned int *fail[2];               // failure bitmaps, 1 bit per base position of a batch
    size_t fail_words;
    int64_t growths;
    hipStream_t stream;                  // stream of the last call that queued work
  };

template <class SLOT>
__global__ void __launch_bounds__(KT_BLOCK) kt_fill_kernel(SLOT *tab, unsigned long long n)
{ for (unsigned long long s = (unsigned long long)blockIdx.x*blockDim.x+threadIdx.x; s < n;
       s += (unsigned long long)gridDim.x*blockDim.x)
    { SLOT e = {};
      e.hi = e.lo = KT_EMPTY;
      tab[s] = e;
    }
}

// every occupied slot of `old` into `tab` (distinct keys: each lane claims a slot of its own, then stores its payload)
template <class SLOT, class CTL>
__global__ void __launch_bounds__(KT_BLOCK) kt_rehash_kernel(const SLOT *old, unsigned long long n_old, SLOT *tab,
                                                             unsigned long long mask, CTL *ctl)
{ unsigned long long nfail = 0;
  for (unsigned long long s = (unsigned long long)blockIdx.x*blockDim.x+threadIdx.x; s < n_old;
       s += (unsigned long long)gridDim.x*blockDim.x)
    { const SLOT o = old[s];
      if (o.lo == KT_EMPTY) continue;
      bool claimed = false;
      SLOT *e = kt_find_or_claim(tab,mask,o.hi,o.lo,&claimed);
      if (!e || !claimed) { nfail++; continue; }
      // The payload, member by member and here: a copy function of the slot type that is handed `o` keeps `o` in memory
      // until it is inlined; the loop then fetches both key words of every slot, empty or not, before it looks at lo,
      // gains two moves, and a table that grows twice while 0.4 Gbases are added takes 0.7 % longer to build
      // (profiles/table_core_ab.txt).
      if constexpr (std::is_array<decltype(SLOT::cnt)>::value)
        { e->cnt[0] = o.cnt[0]; e->cnt[1] = o.cnt[1]; e->cnt[2] = o.cnt[2]; e->cnt[3] = o.cnt[3]; }
      else e->cnt = o.cnt;
    }
  if (nfail) atomicAdd(&ctl->n_rfail,nfail);
}

// a new table of `slots` empty slots (the fill is queued on st)
template <class SLOT>
static int kt_alloc_table(const char *name, SLOT **out, unsigned long long slots, hipStream_t st)
{ void *p = nullptr;
  hipError_t e = hipMalloc(&p,(size_t)slots*sizeof(SLOT));
  if (e != hipSuccess)
    { (void)hipGetLastError();
      char m[160];
      snprintf(m,sizeof(m),"%s: hipMalloc(%llu slots, %llu bytes): %s",name,slots,
               (unsigned long long)(slots*sizeof(SLOT)),hipGetErrorString(e));
      return set_err(CP_ENOMEM,m);
    }
  kt_fill_kernel<<<kt_grid(slots),KT_BLOCK,0,st>>>((SLOT *)p,slots);
  *out = (SLOT *)p;
  return CP_OK;
}

template <class SLOT, class CTL>
static int kt_sync_ctl(kt_store<SLOT,CTL> *t, hipStream_t st)
{ HIPCHK(hipMemcpyAsync(t->h_ctl,t->ctl,sizeof(CTL),hipMemcpyDeviceToHost,st));
  HIPCHK(hipStreamSynchronize(st));
  return CP_OK;
}

// rehash into a table of at least `want` slots (a power of two, > slots); the old table stays intact on failure
template <class SLOT, class CTL>
static int kt_grow(kt_store<SLOT,CTL> *t, unsigned long long want, hipStream_t st)
{ for (int attempt = 0; attempt < 4; attempt++, want <<= 1)
    { SLOT *nt = nullptr;
      int rc = kt_alloc_table(t->name,&nt,want,st);
      if (rc != CP_OK) return rc;
      HIPCHK(hipMemsetAsync(&t->ctl->n_rfail,0,sizeof(unsigned long long),st));
      kt_rehash_kernel<<<kt_grid(t->slots),KT_BLOCK,0,st>>>((const SLOT *)t->tab,t->slots,nt,want-1,t->ctl);
      HIPCHK(hipGetLastError());
      rc = kt_sync_ctl(t,st);
      if (rc != CP_OK) { (void)hipFree(nt); return rc; }
      if (t->h_ctl->n_rfail == 0)
        { HIPCHK(hipFree(t->tab));
          t->tab = nt;
          t->slots = want;
          t->growths++;
          return CP_OK;
        }
      HIPCHK(hipFree(nt));                                 // a probe run too long in the new table: larger still
    }
  return set_err(CP_ENOMEM,std::string(t->name)+": rehash kept failing its probe bound");
}

// the device side of a zero-initialised store: control block and a table of initial_slots (0: the default, 2^20).
// On failure the caller destroys the store.
template <class SLOT, class CTL>
static int kt_init(kt_store<SLOT,CTL> *t, const char *name, int K, int64_t initial_slots)
{ t->name = name;
  t->K = K;
  t->slots = kt_pow2_at_least(initial_slots > 0 ? (unsigned long long)initial_slots : (1ull << 20));
  hipError_t e = hipGetDevice(&t->device);
  if (e == hipSuccess) e = hipMalloc(&t->ctl,sizeof(CTL));
  if (e == hipSuccess) e = hipHostMalloc(&t->h_ctl,sizeof(CTL),hipHostMallocDefault);
  if (e == hipSuccess) e = hipMemset(t->ctl,0,sizeof(CTL));
  if (e == hipSuccess)
    { const int rc = kt_alloc_table(name,&t->tab,t->slots,nullptr);
      if (rc != CP_OK) return rc;
      e = hipStreamSynchronize(nullptr);
    }
  if (e != hipSuccess) return set_err(CP_EHIP,std::string(name)+"_create: "+hipGetErrorString(e));
  return CP_OK;
}

template <class SLOT, class CTL>
static void kt_free(kt_store<SLOT,CTL> *t)
{ (void)hipDeviceSynchronize();
  if (t->tab) (void)hipFree(t->tab);
  if (t->ctl) (void)hipFree(t->ctl);
  if (t->h_ctl) (void)hipHostFree(t->h_ctl);
  for (int i = 0; i < 2; i++)
    if (t->fail[i]) (void)hipFree(t->fail[i]);
}

// two failure bitmaps of at least `words` words
template <class SLOT, class CTL>
static int kt_ensure_bitmaps(kt_store<SLOT,CTL> *t, size_t words, hipStream_t st)
{ if (words <= t->fail_words) return CP_OK;
  HIPCHK(hipStreamSynchronize(st));
  for (int i = 0; i < 2; i++)
    { if (t->fail[i]) { (void)hipFree(t->fail[i]); t->fail[i] = nullptr; }
      if (hipMalloc(&t->fail[i],words*4) != hipSuccess)
        { (void)hipGetLastError();
          t->fail_words = 0;
          return set_err(CP_ENOMEM,std::string(t->name)+"_add: cannot allocate the failure bitmap");
        }
    }
  t->fail_words = words;
  return CP_OK;
}

// An EMPTY table that has fewer than `want` slots (a power of two) is replaced by one of `want`: nothing to rehash, not a
// growth step.  When the allocation fails the table stays and the usual growth takes over.
template <class SLOT, class CTL>
static int kt_presize(kt_store<SLOT,CTL> *t, unsigned long long want, hipStream_t st)
{ SLOT *nt = nullptr;
  if (want > t->slots && kt_alloc_table(t->name,&nt,want,st) == CP_OK)
    { HIPCHK(hipStreamSynchronize(st));
      HIPCHK(hipFree(t->tab));
      t->tab = nt;
      t->slots = want;
    }
  return CP_OK;
}

// Adds a batch of total_bases base positions on st.  launch(replay, fail_in, fail_out) queues the table's add kernel
// over the batch: every position (replay false, fail_in null) or only those whose bit is set in fail_in; a failed
// insert sets its position's bit in fail_out.  *presize (the count table's first-batch sizing; null: never): the first
// batch into a table of the default size gets room for every k-mer of the batch at half load, so that it does not run
// through a table it cannot fit into (each failed insert costs KT_PROBE probes and a replay).  The table is empty then,
// so there is nothing to rehash; when the allocation fails the usual growth takes over.  fail_is_new: a failed insert
// is, nearly always, a key the table does not hold yet, so the growth makes room for the failures too.  The mark pass of
// a filtered count table passes false: its failures are second and later occurrences, many per key, and room for each
// of them would give back the memory that table exists to save; it grows by doubling.
template <class SLOT, class CTL, class F>
static int kt_add(kt_store<SLOT,CTL> *t, int64_t total_bases, hipStream_t st, bool *presize, F launch,
                  bool fail_is_new = true)
{ t->stream = st;
  const size_t words = (size_t)((total_bases+31)/32);
  int rc = kt_ensure_bitmaps(t,words,st);
  if (rc != CP_OK) return rc;
  if (presize && *presize)
    { *presize = false;
      rc = kt_presize(t,kt_pow2_at_least(2*(unsigned long long)total_bases),st);
      if (rc != CP_OK) return rc;
    }
  HIPCHK(hipMemsetAsync(t->fail[0],0,words*4,st));
  HIPCHK(hipMemsetAsync(&t->ctl->n_fail,0,sizeof(unsigned long long),st));
  launch(false,(const unsigned int *)nullptr,t->fail[0]);
  HIPCHK(hipGetLastError());
  // the one read-back: failed inserts and occupancy.  Failures: grow, replay only them; then keep the load <= 1/2.
  for (int round = 0; ; round++)
    { rc = kt_sync_ctl(t,st);
      if (rc != CP_OK) return rc;
      const unsigned long long nfail = t->h_ctl->n_fail, nocc = t->h_ctl->n_occ;
      if (nfail == 0 && 2*nocc <= t->slots) return CP_OK;
      if (round >= 16)
        return set_err(CP_ENOMEM,std::string(t->name)+"_add: the table did not settle after 16 growth steps");
      rc = kt_grow(t,std::max(2*t->slots,kt_pow2_at_least(2*(nocc+(fail_is_new ? nfail : 0)))),st);
      if (rc != CP_OK) return rc;
      if (nfail == 0) continue;
      HIPCHK(hipMemsetAsync(t->fail[1],0,words*4,st));
      HIPCHK(hipMemsetAsync(&t->ctl->n_fail,0,sizeof(unsigned long long),st));
      launch(true,(const unsigned int *)t->fail[0],t->fail[1]);
      HIPCHK(hipGetLastError());
      std::swap(t->fail[0],t->fail[1]);
    }
}

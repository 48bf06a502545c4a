// unitig_dump.h -- what the tools that make the unitigs of a table share (tabunitig, tabgraph, tabpath, tabclean): the
// lengths of the unitigs on the host, the line
//   <tool>: <keys> k-mers, <u> unitigs, <bases> bases, <c> circular, longest <L>, N50 <n>
// and the FASTA and GFA writers of unitig_window.h fed from the device.  The sequences, count sums, flags, components and
// links come down in ranges through buffers of a fixed size; the offsets (8 bytes per unitig) are held whole, because the
// N50 needs every length.
#pragma once
#include "gpu_tool.h"
#include "unitig_window.h"

static const int64_t SEQ_BUF = 1 << 24;    // bases held on the host at a time
static const int64_t UTG_BUF = 1 << 20;    // unitigs whose count sums, flags, components, coverage and link offsets are held at a time
static const int64_t LNK_BUF = 1 << 22;    // links, and their support, held on the host at a time
static const DumpCaps DUMP_CAPS = { SEQ_BUF, UTG_BUF, LNK_BUF };

struct DevFetch
  { template <class T> void operator()(T *dst, const T *src, int64_t first, int64_t count) const
    { HCHK(hipMemcpy(dst,src+first,(size_t)count*sizeof(T),hipMemcpyDeviceToHost)); }
  };

// off[0..count] of the unitigs U down from the device, and len[u] = the bases of unitig u
inline void unitig_lengths(const cp_unitigs *U, std::vector<int64_t> &off, std::vector<int64_t> &len)
{ const int64_t count = cp_unitigs_count(U);
  const int64_t *d_off;
  if (cp_unitigs_arrays(U,nullptr,&d_off,nullptr,nullptr) != CP_OK) cp_die(CP_EINVAL,"cp_unitigs_arrays");
  off.assign((size_t)count+1,0);
  len.resize((size_t)count);
  if (count > 0) HCHK(hipMemcpy(off.data(),d_off,(size_t)(count+1)*8,hipMemcpyDeviceToHost));
  for (int64_t u = 0; u < count; u++) len[(size_t)u] = off[(size_t)u+1]-off[(size_t)u];
}

// the line above on stdout for the unitigs of these lengths, with the tally of the call that made them
inline void print_unitig_line(const std::vector<int64_t> &len, const int64_t *tally)
{ const int64_t n50 = cp_unitig_n50(len.data(),(int64_t)len.size());
  if (n50 < 0) cp_die((int)n50,"cp_unitig_n50");
  printf("%s: %lld k-mers, %lld unitigs, %lld bases, %lld circular, longest %lld, N50 %lld\n",PROG,(long long)tally[CP_UTG_KEYS],
         (long long)tally[CP_UTG_UNITIGS],(long long)tally[CP_UTG_BASES],(long long)tally[CP_UTG_CIRCULAR],
         (long long)tally[CP_UTG_LONGEST],(long long)n50);
}

// ... for tools that need the offsets for nothing else
inline void print_unitig_line(const cp_unitigs *U, const int64_t *tally)
{ std::vector<int64_t> off, len;
  unitig_lengths(U,off,len);
  print_unitig_line(len,tally);
}

// <path>.unitigs.fa of tabunitig: the unitigs U, whose offsets are off
inline bool write_unitig_fasta(FILE *f, const cp_unitigs *U, const std::vector<int64_t> &off)
{ UnitigArrays a = {};
  if (cp_unitigs_arrays(U,&a.seq,nullptr,&a.kc,&a.flag) != CP_OK) cp_die(CP_EINVAL,"cp_unitigs_arrays");
  return write_unitig_fasta(f,cp_unitigs_count(U),off.data(),a,DevFetch(),DUMP_CAPS);
}

// the GFA of tabgraph; with d_cov (per unitig) and d_sup (per link) the RC:i: tags of tabpath as well
inline bool write_gfa(FILE *f, const cp_unitigs *U, const cp_unitig_graph *G, int K, const std::vector<int64_t> &off,
                      const int64_t *d_cov, const int64_t *d_sup)
{ UnitigArrays a = {};
  if (cp_unitigs_arrays(U,&a.seq,nullptr,&a.kc,nullptr) != CP_OK) cp_die(CP_EINVAL,"cp_unitigs_arrays");
  if (cp_unitig_graph_arrays(G,&a.loff,&a.link,nullptr,&a.comp) != CP_OK) cp_die(CP_EINVAL,"cp_unitig_graph_arrays");
  a.cov = d_cov;
  a.sup = d_sup;
  return write_gfa(f,K,cp_unitigs_count(U),cp_unitig_graph_links(G),off.data(),a,DevFetch(),DUMP_CAPS);
}

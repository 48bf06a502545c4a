// class_batch.h -- a .class file on the device, batch by batch (class2cns, class2ktab): the pinned host and device
// buffers that class_record.h's for_class_batches fills, and the label table (cp_kmer_table_*, include/classpro_amd.h)
// of a whole file.
#pragma once
#include "gpu_tool.h"
#include "class_record.h"

static const int64_t CLASS_BATCH_BASES = (int64_t)256 << 20; // bases per device batch
static const int64_t CLASS_BATCH_READS = 1 << 16;            // and reads

// host and device buffers of one batch of records (pinned host memory), of exactly the size asked for
struct ClassBatch
  { char *h_seq = nullptr, *h_lab = nullptr, *d_seq = nullptr, *d_lab = nullptr;
    int64_t *h_off = nullptr, *d_off = nullptr;
    int64_t cap_bases = 0, cap_reads = 0, nbases = 0;
    int nreads = 0;

    void reserve(int64_t bases, int64_t reads)
    { if (bases > cap_bases)
        { if (h_seq) { HCHK(hipHostFree(h_seq)); HCHK(hipHostFree(h_lab)); HCHK(hipFree(d_seq)); HCHK(hipFree(d_lab)); }
          HCHK(hipHostMalloc((void **)&h_seq,bases,hipHostMallocDefault));
          HCHK(hipHostMalloc((void **)&h_lab,bases,hipHostMallocDefault));
          HCHK(hipMalloc((void **)&d_seq,bases));
          HCHK(hipMalloc((void **)&d_lab,bases));
          cap_bases = bases;
        }
      if (reads+1 > cap_reads)
        { if (h_off) { HCHK(hipHostFree(h_off)); HCHK(hipFree(d_off)); }
          HCHK(hipHostMalloc((void **)&h_off,(reads+1)*8,hipHostMallocDefault));
          HCHK(hipMalloc((void **)&d_off,(reads+1)*8));
          cap_reads = reads+1;
        }
    }
    void upload()
    { HCHK(hipMemcpy(d_seq,h_seq,nbases,hipMemcpyHostToDevice));
      HCHK(hipMemcpy(d_lab,h_lab,nbases,hipMemcpyHostToDevice));
      HCHK(hipMemcpy(d_off,h_off,(nreads+1)*8,hipMemcpyHostToDevice));
    }
    void release()
    { if (h_seq) { HCHK(hipHostFree(h_seq)); HCHK(hipHostFree(h_lab)); HCHK(hipFree(d_seq)); HCHK(hipFree(d_lab)); }
      if (h_off) { HCHK(hipHostFree(h_off)); HCHK(hipFree(d_off)); }
      h_seq = h_lab = d_seq = d_lab = nullptr;
      h_off = d_off = nullptr;
      cap_bases = cap_reads = 0;
    }
  };

// The label table of every record of cls_path, on GPU 0 (the first device work of the tool), and its statistics, which
// end the run on a label other than E/H/D/R; -v says what was added.  B keeps its buffers for the caller.
static cp_kmer_table *fill_label_table(const char *cls_path, int K, bool canonical, bool verbose, ClassBatch &B,
                                       cp_kmer_stats *st)
{ HCHK(hipSetDevice(0));
  cp_kmer_table *T = nullptr;
  int rc = cp_kmer_table_create(K,canonical ? 1 : 0,0,&T);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_table_create");
  for_class_batches(cls_path,B,CLASS_BATCH_BASES,CLASS_BATCH_READS,false,
                    [&](ClassBatch &b, std::vector<std::string> &)
    { b.upload();
      const int r = cp_kmer_table_add(T,b.d_seq,b.d_off,b.d_lab,b.nreads,b.nbases,nullptr);
      if (r != CP_OK) cp_die(r,"cp_kmer_table_add");
      HCHK(hipStreamSynchronize(nullptr));                          // the host buffers are refilled next
    });
  rc = cp_kmer_table_stats(T,st);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_table_stats");
  if (verbose)
    fprintf(stderr,"%s: K = %d%s: %lld k-mer positions, %lld distinct k-mers, %lld unanimous, %lld skipped "
                   "(a base other than A C G T); table %lld slots, %.3f GB, %lld growth steps\n",
            PROG,K,canonical ? " canonical" : "",(long long)st->n_kmers,(long long)st->n_distinct,
            (long long)st->n_unanimous,(long long)st->n_skipped,(long long)st->slots,st->bytes/1e9,
            (long long)st->growths);
  return T;
}

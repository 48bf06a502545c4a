// class_batch_check.cpp -- test harness (CPU): the batch loop over a .class file that class2cns and class2ktab share
// (classpro_amd/csrc/host/class_record.h for_class_batches), driven with heap buffers of exactly the size asked for,
// so that AddressSanitizer sees every byte past a capacity.
//   class_batch_check <file.class[.gz]> <batch_bases> <batch_reads>
// Prints "B <nreads> <nbases>" for every batch, then its records as "@header\nseq\n+\nlabels\n".
#include <cstdio>
#include <cstdlib>
#include "../classpro_amd/csrc/host/class_record.h"

struct HeapBatch
  { char *h_seq = nullptr, *h_lab = nullptr;
    int64_t *h_off = nullptr;
    int64_t cap_bases = 0, cap_reads = 0, nbases = 0;
    int nreads = 0;

    void reserve(int64_t bases, int64_t reads)                      // as ClassBatch::reserve: frees, never copies
    { if (bases > cap_bases)
        { free(h_seq); free(h_lab);
          h_seq = (char *)malloc((size_t)bases);
          h_lab = (char *)malloc((size_t)bases);
          cap_bases = bases;
        }
      if (reads+1 > cap_reads)
        { free(h_off);
          h_off = (int64_t *)malloc((size_t)(reads+1)*8);
          cap_reads = reads+1;
        }
    }
    ~HeapBatch() { free(h_seq); free(h_lab); free(h_off); }
  };

int main(int argc, char **argv)
{ PROG = "class_batch_check";
  if (argc != 4) { fprintf(stderr,"Usage: %s <file.class[.gz]> <batch_bases> <batch_reads>\n",PROG); return 2; }
  HeapBatch B;
  for_class_batches(argv[1],B,atoll(argv[2]),atoll(argv[3]),true,[](HeapBatch &b, std::vector<std::string> &headers)
    { printf("B %d %lld\n",b.nreads,(long long)b.nbases);
      if (headers.size() != (size_t)b.nreads || b.h_off[0] != 0 || b.h_off[b.nreads] != b.nbases)
        { printf("BAD BATCH: %zu headers, offsets %lld .. %lld\n",headers.size(),(long long)b.h_off[0],
                 (long long)b.h_off[b.nreads]);
          exit(1);
        }
      for (int i = 0; i < b.nreads; i++)
        { const int64_t s = b.h_off[i], n = b.h_off[i+1]-s;
          write_class_record(stdout,headers[(size_t)i],b.h_seq+s,(size_t)n,b.h_lab+s,(size_t)n);
        }
    });
  return 0;
}

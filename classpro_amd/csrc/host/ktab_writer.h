// ktab_writer.h -- writes a FASTK k-mer table (layout: classpro_amd/fastk.py) from a sorted snapshot on the device
// (cp_kmer_sorted, "Sorted k-mers" in include/classpro_amd.h): the stub <root>.ktab with K, nparts, minval, ibyte and
// the prefix index, and the parts .<root>.ktab.1..n (kprof -t, class2ktab).  Part p of nparts = max(1, min(threads,
// entries)) holds the entries [entries*p/nparts, entries*(p+1)/nparts).  The records are encoded on the device and come
// down in ranges of TAB_RANGE entries through one buffer that a writer keeps from table to table; the host only writes.
#pragma once
#include "gpu_tool.h"

static const int64_t TAB_RANGE = (int64_t)4 << 20;           // table entries per transfer (records of at most 15 bytes: 60 MiB)

struct KtabWriter
  { DevBuf<uint8_t> d_rec;
    std::vector<uint8_t> h_rec;
    int64_t entries = 0;                                             // of the table written last
    int ibyte = 0, nparts = 0;

    // writes the stub to ft (opened by the tool as tab_path before the GPU is touched), then the parts beside it
    void write(cp_kmer_sorted *sorted, int K, int minval, int nthreads, FILE *ft, const std::string &tab_path,
               const std::string &odir, const std::string &oname)
    { int rc;
      entries = cp_kmer_sorted_size(sorted);
      ibyte = cp_ktab_ibyte(K);
      const int pbyte = ((K+3) >> 2)-ibyte+2;
      nparts = (int)std::max<int64_t>(1,std::min<int64_t>(nthreads,entries));
      { std::vector<int64_t> index((size_t)1 << (8*ibyte));
        DevBuf<int64_t> d_index;
        d_index.need(index.size());
        rc = cp_kmer_sorted_ktab(sorted,0,0,nullptr,d_index.p,nullptr);
        if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_ktab");
        HCHK(hipMemcpy(index.data(),d_index.p,index.size()*8,hipMemcpyDeviceToHost));
        d_index.release();
        const bool ok = fwrite(&K,4,1,ft) == 1 && fwrite(&nparts,4,1,ft) == 1 && fwrite(&minval,4,1,ft) == 1
                        && fwrite(&ibyte,4,1,ft) == 1 && fwrite(index.data(),8,index.size(),ft) == index.size();
        if (fclose(ft) != 0 || !ok) die("%s: Cannot write %s\n",PROG,tab_path.c_str());
      }
      for (int p = 0; p < nparts; p++)
        { const int64_t e0 = entries*p/nparts, e1 = entries*(p+1)/nparts, nels = e1-e0;
          const std::string part = odir+"/."+oname+".ktab."+std::to_string(p+1);
          FILE *fp = fopen(part.c_str(),"wb");
          if (!fp) die("%s: Cannot open %s for 'w'\n",PROG,part.c_str());
          bool ok = fwrite(&K,4,1,fp) == 1 && fwrite(&nels,8,1,fp) == 1;
          for (int64_t e = e0; e < e1 && ok; e += TAB_RANGE)
            { const int64_t m = std::min(TAB_RANGE,e1-e);
              d_rec.need((size_t)(m*pbyte));
              h_rec.resize((size_t)(m*pbyte));
              rc = cp_kmer_sorted_ktab(sorted,e,m,d_rec.p,nullptr,nullptr);
              if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_ktab");
              HCHK(hipMemcpy(h_rec.data(),d_rec.p,h_rec.size(),hipMemcpyDeviceToHost));
              ok = fwrite(h_rec.data(),1,h_rec.size(),fp) == h_rec.size();
            }
          if (fclose(fp) != 0 || !ok) die("%s: Cannot write %s\n",PROG,part.c_str());
        }
    }
    // gives the transfer buffer back
    void release() { d_rec.release(); }
  };

// ktab_reader.h -- reads a FASTK k-mer table (layout: classpro_amd/fastk.py): the stub <root>.ktab with K, nparts,
// minval, ibyte and the prefix index, and the records of the parts .<root>.ktab.1..n in file order (tab2prof).  open()
// checks everything that can be checked without decoding a key, so that a tool can refuse a bad table before it touches
// the GPU; read() then hands the records out in pieces, across part boundaries.  The records are not decoded here: the
// device does that (cp_kmer_sorted_load_records).  Plain C++; no device code.
//
// open() ends the tool with exit status 1 and one of these lines on stderr:
//   <prog>: Cannot open <stub> [errno=<n>]
//   <prog>: <stub> is truncated                                                   no header, or a short index
//   <prog>: K-mer length of <stub> must lie in [5, 63] (<K>)
//   <prog>: <stub> has <ibyte> prefix bytes, a table of <K>-mers has <n>
//   <prog>: <stub> names no parts (<nparts>)
//   <prog>: The index of <stub> is negative or decreases at prefix <p>
//   <prog>: Table part <part> is missing
//   <prog>: Table part <part> is truncated                                        no header
//   <prog>: Table part <part> does not have the k-mer length of the stub (<k> vs <K>)
//   <prog>: Table part <part> holds <size> bytes, its <nels> records of <pbyte> bytes need <want>
//   <prog>: The parts of <stub> hold <sum> entries, its index ends at <n>
#pragma once
#include <sys/stat.h>
#include <algorithm>
#include "host_io.h"

static int ktab_ibyte(int K)                                         // the rule of cp_ktab_ibyte
{ return K >= 13 ? 3 : K >= 9 ? 2 : K >= 5 ? 1 : 0; }

struct KtabReader
  { int K = 0, nparts = 0, minval = 0, ibyte = 0, pbyte = 0;
    int64_t entries = 0;
    std::string stub;
    std::vector<int64_t> index;                                      // 1 << 8*ibyte cells
    std::vector<std::string> part;
    std::vector<int64_t> nels;
    int cur = -1;                                                    // read(): the part being read
    int64_t left = 0;                                                // and its records still to come
    FILE *f = nullptr;

    ~KtabReader() { if (f) fclose(f); }

    // `name` is <dir>/<root>[.ktab]
    void open(const std::string &name)
    { const std::string dir = path_to(name), root = root_of(name,".ktab");
      stub = dir+"/"+root+".ktab";
      FILE *s = fopen(stub.c_str(),"rb");
      if (!s) die("%s: Cannot open %s [errno=%d]\n",PROG,stub.c_str(),errno);
      int head[4];
      if (fread(head,4,4,s) != 4) { fclose(s); die("%s: %s is truncated\n",PROG,stub.c_str()); }
      K = head[0]; nparts = head[1]; minval = head[2]; ibyte = head[3];
      if (K < 5 || K > 63) { fclose(s); die("%s: K-mer length of %s must lie in [5, 63] (%d)\n",PROG,stub.c_str(),K); }
      if (ibyte != ktab_ibyte(K))
        { fclose(s);
          die("%s: %s has %d prefix bytes, a table of %d-mers has %d\n",PROG,stub.c_str(),ibyte,K,ktab_ibyte(K));
        }
      if (nparts < 1) { fclose(s); die("%s: %s names no parts (%d)\n",PROG,stub.c_str(),nparts); }
      index.resize((size_t)1 << (8*ibyte));
      const bool whole = fread(index.data(),8,index.size(),s) == index.size();
      fclose(s);
      if (!whole) die("%s: %s is truncated\n",PROG,stub.c_str());
      int64_t before = 0;
      for (size_t p = 0; p < index.size(); p++)
        { if (index[p] < before) die("%s: The index of %s is negative or decreases at prefix %zu\n",PROG,stub.c_str(),p);
          before = index[p];
        }
      pbyte = ((K+3) >> 2)-ibyte+2;
      part.resize((size_t)nparts);
      nels.resize((size_t)nparts);
      entries = 0;
      for (int p = 0; p < nparts; p++)
        { const std::string &nm = part[(size_t)p] = dir+"/."+root+".ktab."+std::to_string(p+1);
          FILE *g = fopen(nm.c_str(),"rb");
          if (!g) die("%s: Table part %s is missing\n",PROG,nm.c_str());
          int k;
          int64_t n;
          const bool ok = fread(&k,4,1,g) == 1 && fread(&n,8,1,g) == 1;
          struct stat st;
          const bool sized = fstat(fileno(g),&st) == 0;
          fclose(g);
          if (!ok || !sized) die("%s: Table part %s is truncated\n",PROG,nm.c_str());
          if (k != K) die("%s: Table part %s does not have the k-mer length of the stub (%d vs %d)\n",PROG,nm.c_str(),k,K);
          if (n < 0 || n > ((int64_t)1 << 56) || (int64_t)st.st_size != 12+n*pbyte)
            die("%s: Table part %s holds %lld bytes, its %lld records of %d bytes need %lld\n",PROG,nm.c_str(),
                (long long)st.st_size,(long long)n,pbyte,(long long)(12+n*pbyte));
          nels[(size_t)p] = n;
          entries += n;
        }
      if (entries != index.back())
        die("%s: The parts of %s hold %lld entries, its index ends at %lld\n",PROG,stub.c_str(),(long long)entries,
            (long long)index.back());
      cur = -1;
      left = 0;
    }

    // the next records, at most max_entries of them, into dst (max_entries * pbyte bytes); returns how many, 0 at the end
    int64_t read(uint8_t *dst, int64_t max_entries)
    { int64_t got = 0;
      while (got < max_entries)
        { if (left == 0)
            { if (f) { fclose(f); f = nullptr; }
              if (cur+1 >= nparts) break;
              const std::string &nm = part[(size_t)++cur];
              f = fopen(nm.c_str(),"rb");
              if (!f || fseek(f,12,SEEK_SET) != 0) die("%s: Table part %s is missing\n",PROG,nm.c_str());
              left = nels[(size_t)cur];
              continue;
            }
          const int64_t m = std::min(left,max_entries-got);
          if (fread(dst+got*pbyte,(size_t)pbyte,(size_t)m,f) != (size_t)m)
            die("%s: Table part %s changed while it was read\n",PROG,part[(size_t)cur].c_str());
          got += m;
          left -= m;
        }
      return got;
    }
  };

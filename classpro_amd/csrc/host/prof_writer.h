// prof_writer.h -- writes FASTK count profiles (layout: classpro_amd/fastk.py): the stub <root>.prof and the parts
// .<root>.prof.1..n with their indices .<root>.pidx.1..n (kprof, genome2class -p).  Part p of nparts holds the reads
// [reads*p/nparts, reads*(p+1)/nparts).  The reads come in order, batch by batch; the tool encodes a batch's profiles
// on its threads (cp_encode_profile), each into clen and a buffer of its own, then appends them here.
#pragma once
#include "host_io.h"

struct Part
  { FILE *f = nullptr;
    std::string name;
    int64_t first = 0, n = 0, bytes = 0;
    std::vector<int64_t> ends;
  };

struct ProfWriter
  { int K = 0;
    std::string odir, oname;
    std::vector<Part> parts;
    std::vector<int64_t> clen;                                       // per read of the batch: bytes of its code
    int64_t done = 0;                                                // reads written so far
    int part = 0;

    // writes the stub to fs (opened by the tool as stub_path before the GPU is touched) and opens the parts
    void open(FILE *fs, const std::string &stub_path, int kmer, int nparts, int64_t nreads, const std::string &dir,
              const std::string &name)
    { K = kmer; odir = dir; oname = name;
      if (fwrite(&K,4,1,fs) != 1 || fwrite(&nparts,4,1,fs) != 1 || fclose(fs) != 0)
        die("%s: Cannot write %s\n",PROG,stub_path.c_str());
      parts.resize((size_t)nparts);
      for (int p = 0; p < nparts; p++)
        { Part &P = parts[(size_t)p];
          P.first = nreads*p/nparts;
          P.n = nreads*(p+1)/nparts-P.first;
          P.name = odir+"/."+oname+".prof."+std::to_string(p+1);
          P.f = fopen(P.name.c_str(),"wb");
          if (!P.f) die("%s: Cannot open %s for 'w'\n",PROG,P.name.c_str());
          P.ends.reserve((size_t)P.n);
        }
    }
    // the codes of the batch's reads [r0, r1), one after the other in `code`, to the parts they belong to
    void append(int r0, int r1, const uint8_t *code)
    { int64_t o = 0;
      for (int r = r0; r < r1; r++, done++)
        { while (done >= parts[(size_t)part].first+parts[(size_t)part].n) part++;
          Part &P = parts[(size_t)part];
          const int64_t l = clen[(size_t)r];
          if (l > 0 && fwrite(code+o,1,(size_t)l,P.f) != (size_t)l)
            die("%s: Cannot write %s\n",PROG,P.name.c_str());
          o += l;
          P.bytes += l;
          P.ends.push_back(P.bytes);
        }
    }
    void close()
    { for (size_t p = 0; p < parts.size(); p++)
        { Part &P = parts[p];
          if (fclose(P.f) != 0) die("%s: Cannot write %s\n",PROG,P.name.c_str());
          const std::string nm = odir+"/."+oname+".pidx."+std::to_string(p+1);
          FILE *f = fopen(nm.c_str(),"wb");
          if (!f) die("%s: Cannot open %s for 'w'\n",PROG,nm.c_str());
          bool ok = fwrite(&K,4,1,f) == 1 && fwrite(&P.first,8,1,f) == 1 && fwrite(&P.n,8,1,f) == 1
                    && (P.n == 0 || fwrite(P.ends.data(),8,(size_t)P.n,f) == (size_t)P.n);
          if (fclose(f) != 0 || !ok) die("%s: Cannot write %s\n",PROG,nm.c_str());
        }
    }
  };

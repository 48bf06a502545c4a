// class_record.h -- the header of a FASTX read as the reference's tools print it, one record of a .class file for every
// tool that writes one, and the batch loop over a .class file for the tools that read one (class2cns, class2ktab).
// Plain C++; no device code.
#pragma once
#include <cerrno>
#include "host_io.h"

static const int CLASS_FASTX_RLEN_MAX = 60000;               // prof2class.c:154-160: the bound for FASTX sources

// "@name comment"; kseq keeps the previous comment buffer, and a source without any comment so far prints "(null)"
static std::string fastx_class_header(const FastxReader &fx)
{ return "@"+fx.name+" "+(fx.have_comment ? fx.comment : std::string("(null)")); }

// the read's name in a .class header: the text between '@' and the first space
static std::string class_header_name(const std::string &header)
{ const size_t sp = header.find(' ');
  return header.substr(1,sp == std::string::npos ? std::string::npos : sp-1);
}

// "@header\nseq\n+\nlabels\n"
static void write_class_record(FILE *out, const std::string &header, const char *seq, size_t rlen, const char *labels,
                               size_t nlabels)
{ fputs(header.c_str(),out); fputc('\n',out);
  fwrite(seq,1,rlen,out);
  fputs("\n+\n",out);
  fwrite(labels,1,nlabels,out);
  fputc('\n',out);
}

// Reads the records of the .class file `path` in batches of at most batch_bases bases and batch_reads reads and calls
// f(B, headers) for each; a record longer than batch_bases gets a batch of its own, and B keeps the larger capacity.
// B provides reserve(bases, reads) -- room for that many bases in h_seq and h_lab and for reads+1 offsets in h_off,
// never less than it has, contents not kept -- and cap_bases, cap_reads (offsets), nbases, nreads.  Record i of a batch
// is h_seq / h_lab [h_off[i], h_off[i+1]); headers[i] is its "@name[ comment]" when keep_headers is set, and the vector
// is empty otherwise.
template <class Buf, class F>
static void for_class_batches(const char *path, Buf &B, int64_t batch_bases, int64_t batch_reads, bool keep_headers, F f)
{ FastxReader in(path);
  if (!in.f) die("%s: Cannot open %s [errno=%d]\n",PROG,path,errno);
  std::vector<std::string> headers;
  B.reserve(batch_bases,batch_reads);
  B.nreads = 0; B.nbases = 0; B.h_off[0] = 0;
  auto flush = [&]()
    { if (B.nreads) f(B,headers);
      B.nreads = 0; B.nbases = 0; B.h_off[0] = 0;
      headers.clear();
    };
  while (in.next() >= 0)
    { const int64_t n = (int64_t)in.seq.size();
      if (in.qual.size() != in.seq.size())
        die("%s: record %s of %s carries no labels\n",PROG,in.name.c_str(),path);
      if (B.nbases+n > B.cap_bases || B.nreads+1 >= B.cap_reads) flush();
      if (n > B.cap_bases) B.reserve(n,B.cap_reads-1);             // the offsets keep their buffer, and h_off[0] its 0
      memcpy(B.h_seq+B.nbases,in.seq.data(),n);
      memcpy(B.h_lab+B.nbases,in.qual.data(),n);
      B.nbases += n;
      B.h_off[++B.nreads] = B.nbases;
      if (keep_headers)
        headers.push_back("@"+in.name+(in.rec_comment ? " "+in.comment : std::string()));
    }
  flush();
}

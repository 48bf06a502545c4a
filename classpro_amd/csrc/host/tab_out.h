// tab_out.h -- what the tools that work on k-mer tables and write files of their own share (tabop, tabhet, tabunitig,
// tabgraph, tabpath, tabclean): the outputs created before the GPU is touched, the check that a result table is not an
// operand, a table brought up on the device, and a stop watch.
#pragma once
#include <sys/stat.h>
#include <chrono>
#include "gpu_tool.h"
#include "ktab_upload.h"

// The output files of a tool, created before the GPU is touched so that a name that cannot be written costs no GPU work.
// They are made in the order the tool asks for them, each opened and truncated before the next is opened.  (tabop and
// tabclean used to open the table and the histogram before truncating either: the message names another file only when
// the table's ftruncate and the histogram's open fail in the same run.)  On the first path that cannot be made every file
// made so far is closed, those that did not exist before are removed again, and the tool ends.  A file that was made is
// the tool's from then on: it writes and closes it.
struct Outputs
  { struct Out { std::string path; FILE *f; bool fresh; };
    std::vector<Out> made;

    FILE *create(const std::string &path)
    { const bool fresh = access(path.c_str(),F_OK) != 0;
      const int fd = open(path.c_str(),O_WRONLY|O_CREAT,0666);
      FILE *f = nullptr;
      if (fd >= 0 && (ftruncate(fd,0) != 0 || !(f = fdopen(fd,"wb")))) close(fd);
      if (!f)
        { for (const Out &o : made)                            // what was created here is removed again
            { fclose(o.f);
              if (o.fresh) unlink(o.path.c_str());
            }
          if (fd >= 0 && fresh) unlink(path.c_str());
          die("%s: Cannot open %s for 'w'\n",PROG,path.c_str());
        }
      made.push_back(Out{ path, f, fresh });
      return f;
    }
  };

// the result may not replace a table it is made from; what = "is the operand" or "is an operand"
inline void die_if_operand(const std::string &tab_path, const std::string &stub, const char *what)
{ struct stat so, si;
  if (tab_path == stub || (stat(tab_path.c_str(),&so) == 0 && stat(stub.c_str(),&si) == 0
                           && so.st_dev == si.st_dev && so.st_ino == si.st_ino))
    die("%s: %s %s: the result needs a name of its own\n",PROG,tab_path.c_str(),what);
}

// the table of an opened reader as a snapshot on device 0; the buffer its records went through is given back
inline cp_kmer_sorted *upload_table(KtabReader &tab)
{ HCHK(hipSetDevice(0));
  DevBuf<uint8_t> d_rec;
  cp_kmer_sorted *T = upload_ktab(tab,d_rec);
  d_rec.release();
  return T;
}

inline double since(std::chrono::steady_clock::time_point t0)
{ return std::chrono::duration<double>(std::chrono::steady_clock::now()-t0).count(); }

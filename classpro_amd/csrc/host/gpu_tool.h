// gpu_tool.h -- what the command-line tools that use the GPU share (ClassGS, class2cns, class2ktab, kprof,
// genome2class, tab2prof, tabbin, tabtrack, tabcmp, and through tab_out.h tabop, tabhet, tabunitig, tabgraph, tabpath and
// tabclean): how a failed library or HIP call ends the tool, a device buffer that only grows until it is given back,
// and the accuracy totals read from the device.  Needs the HIP runtime, so the host-only tools (prof2class, class2acc)
// do not include it.  class_batch.h builds the .class batches of class2cns and class2ktab on it, ktab_upload.h and
// ktab_writer.h the way of a k-mer table onto the device and back, tab_out.h and unitig_dump.h what the table tools share.
#pragma once
#include <hip/hip_runtime.h>
#include "host_io.h"
#include "acc_report.h"
#include "../../../include/classpro_amd.h"

static void cp_die(int rc, const char *what)
{ die("%s: %s: %s (%d)\n",PROG,what,cp_last_error(),rc); }

static void hip_die(hipError_t e, const char *what)
{ die("%s: %s: %s\n",PROG,what,hipGetErrorString(e)); }

#define HCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) hip_die(e_,#call); } while (0)

// a device buffer that only grows, until release() gives it back
template <class T>
struct DevBuf
  { T *p = nullptr;
    size_t cap = 0;
    T *need(size_t n)
    { if (n > cap)
        { if (p) HCHK(hipFree(p));
          cap = n+n/4+64;
          HCHK(hipMalloc((void **)&p,cap*sizeof(T)));
        }
      return p;
    }
    void release()
    { if (p) HCHK(hipFree(p));
      p = nullptr;
      cap = 0;
    }
    void up(const std::vector<T> &h) { need(h.size()+1); if (!h.empty()) HCHK(hipMemcpy(p,h.data(),h.size()*sizeof(T),hipMemcpyHostToDevice)); }
  };

// the counts of a cp_acc, as print_acc_report takes them
static AccTotals acc_totals(cp_acc *acc)
{ cp_acc_stats st;
  const int rc = cp_acc_read(acc,&st);
  if (rc != CP_OK) cp_die(rc,"cp_acc_read");
  AccTotals a;
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) a.cfm[i][j] = st.cfm[i][j];
  a.ntot = st.ntot; a.ncor = st.ncor; a.nfne = st.nfne;
  a.ntot_normal = st.ntot_normal; a.ncor_normal = st.ncor_normal; a.nfne_normal = st.nfne_normal;
  a.ntot_repeat = st.ntot_repeat; a.ncor_repeat = st.ncor_repeat; a.nfne_repeat = st.nfne_repeat;
  return a;
}

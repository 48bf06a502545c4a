// ktab_upload.h -- a FASTK k-mer table from the host onto the device as a sorted snapshot (tab2prof, tabop, tabbin, tabcmp): the
// records of an opened KtabReader go up in pieces of TAB_RANGE entries through one device buffer into
// cp_kmer_sorted_load_records and are checked there (cp_kmer_sorted_load_end: strictly ascending keys; "Sorted k-mers as
// input" in include/classpro_amd.h).  A failed call ends the tool.  The buffer is the caller's, so that several tables
// share it; ktab_reader.h itself stays free of device code.  DevBuf, HCHK and cp_die are gpu_tool.h's; TAB_RANGE, the
// entries per transfer, is the one constant of ktab_writer.h, so that a table goes up in the pieces it comes down in.
#pragma once
#include "gpu_tool.h"
#include "ktab_reader.h"
#include "ktab_writer.h"

static cp_kmer_sorted *upload_ktab(KtabReader &tab, DevBuf<uint8_t> &d_rec)
{ cp_kmer_sorted *T = nullptr;
  int rc = cp_kmer_sorted_load_begin(tab.K,tab.index.data(),&T);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_load_begin");
  std::vector<uint8_t> h_rec((size_t)(std::min(TAB_RANGE,std::max<int64_t>(tab.entries,1))*tab.pbyte));
  int64_t m;
  while ((m = tab.read(h_rec.data(),TAB_RANGE)) > 0)
    { d_rec.need((size_t)(m*tab.pbyte));
      HCHK(hipMemcpy(d_rec.p,h_rec.data(),(size_t)(m*tab.pbyte),hipMemcpyHostToDevice));
      rc = cp_kmer_sorted_load_records(T,m,d_rec.p,nullptr);         // the next copy waits for it: one stream
      if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_load_records");
    }
  rc = cp_kmer_sorted_load_end(T,nullptr);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_load_end");
  return T;
}

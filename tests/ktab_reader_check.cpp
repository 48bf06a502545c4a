// ktab_reader_check.cpp -- test harness (CPU): the reader of a FASTK k-mer table that tab2prof uses
// (classpro_amd/csrc/host/ktab_reader.h), driven with heap buffers of exactly the size asked for, so that
// AddressSanitizer sees every byte past a piece.
//   ktab_reader_check <table>[.ktab] <piece>
// Prints "K nparts minval ibyte pbyte entries\n", then the index and then the records as they are, read in pieces of at
// most <piece> entries, then "pieces <n>\n".  stderr carries nothing but the reader's own messages.
#include <cstdio>
#include <cstdlib>
#include "../classpro_amd/csrc/host/ktab_reader.h"

int main(int argc, char **argv)
{ PROG = "ktab_reader_check";
  if (argc != 3) { fprintf(stderr,"Usage: %s <table>[.ktab] <piece>\n",PROG); return 2; }
  const int64_t piece = atoll(argv[2]);
  KtabReader R;
  R.open(argv[1]);
  printf("%d %d %d %d %d %lld\n",R.K,R.nparts,R.minval,R.ibyte,R.pbyte,(long long)R.entries);
  fwrite(R.index.data(),8,R.index.size(),stdout);
  int64_t done = 0, pieces = 0;
  for (;;)
    { const int64_t ask = std::min(piece,R.entries-done);
      uint8_t *buf = (uint8_t *)malloc((size_t)(ask*R.pbyte)+(ask == 0));     // ask = 0: the read past the end
      const int64_t m = R.read(buf,ask);
      if (m != ask) { printf("\nBAD PIECE: asked %lld, got %lld\n",(long long)ask,(long long)m); return 1; }
      fwrite(buf,(size_t)R.pbyte,(size_t)m,stdout);
      free(buf);
      if (m == 0) break;
      done += m;
      pieces++;
    }
  printf("pieces %lld\n",(long long)pieces);
  return 0;
}

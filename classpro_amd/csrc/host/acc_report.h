// acc_report.h -- the closing report of class2acc (src/class2acc.c:292-316): the 4x4 confusion matrix (truth rows,
// estimate columns, order E R H D) and the overall / [Normal] / [Repeat] accuracy lines.  Shared by class2acc and by
// ClassGS -A, which fills the same numbers from the device counts (cp_acc_read).
#pragma once
#include <cstdio>

struct AccTotals
  { long long cfm[4][4] = {};
    long long ntot = 0, ncor = 0, nfne = 0;
    long long ntot_normal = 0, ncor_normal = 0, nfne_normal = 0;
    long long ntot_repeat = 0, ncor_repeat = 0, nfne_repeat = 0;
  };

static void print_acc_report(FILE *out, const AccTotals &a)
{ static const char stoc[4] = { 'E', 'R', 'H', 'D' };
  fprintf(out,"\nConfusion Matrix (Truth\\Est):\n  ");
  for (int i = 0; i < 4; i++) fprintf(out,"%15c",stoc[i]);
  fprintf(out,"\n");
  for (int i = 0; i < 4; i++)
    { fprintf(out,"%c:",stoc[i]);
      for (int j = 0; j < 4; j++) fprintf(out,"%15lld",a.cfm[i][j]);
      fprintf(out,"\n");
    }
  fprintf(out,"\nAccuracy = %4.2lf %% (= %lld / %lld), FN Error = %4.2lf %%\n",
          (double)a.ncor/a.ntot*100,a.ncor,a.ntot,(double)a.nfne/a.ntot*100);
  fprintf(out,"[Normal] Accuracy = %4.2lf %% (= %lld / %lld), FN Error = %4.2lf %%\n",
          (double)a.ncor_normal/a.ntot_normal*100,a.ncor_normal,a.ntot_normal,(double)a.nfne_normal/a.ntot_normal*100);
  fprintf(out,"[Repeat] Accuracy = %4.2lf %% (= %lld / %lld), FN Error = %4.2lf %%\n",
          (double)a.ncor_repeat/a.ntot_repeat*100,a.ncor_repeat,a.ntot_repeat,(double)a.nfne_repeat/a.ntot_repeat*100);
}

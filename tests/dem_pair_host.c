/* dem_pair_host.c -- ko_dem_pair (oracle/kid_oracle_mts.c) in a program of its own, for AddressSanitizer and
 * UndefinedBehaviorSanitizer: tests/test_dem_pair_cpu.py compiles it together with the oracle's sources, feeds it the edge inputs
 * of tests/dem_pair_ref.py and compares what it prints with what the oracle's shared library returned, bit for bit.
 *   argv[1]: cases, each sizeof(kid_params) bytes, then int64 latlon, int64 id[2], double x[26]
 *   argv[2]: results, 40 doubles per case */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../oracle/kid_oracle.h"

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: dem_pair_host cases results\n"); return 2; }
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
  long ncase = 0;
  for (;;) {
    kid_params *p = (kid_params *)malloc(sizeof(kid_params));   /* (heap copies of exactly the sizes the routine may touch) */
    int64_t *head = (int64_t *)malloc(3 * sizeof(int64_t));
    double *x = (double *)malloc(26 * sizeof(double)), *res = (double *)malloc(40 * sizeof(double));
    if (!p || !head || !x || !res) return 2;
    const size_t got = fread(p, sizeof(kid_params), 1, in);
    if (got == 1 && (fread(head, sizeof(int64_t), 3, in) != 3 || fread(x, sizeof(double), 26, in) != 26)) { fprintf(stderr, "short case\n"); return 2; }
    if (got == 1) {
      ko_dem_pair(p, (int)head[0], head + 1, x, res);
      if (fwrite(res, sizeof(double), 40, out) != 40) return 2;
      ++ncase;
    }
    free(p); free(head); free(x); free(res);
    if (got != 1) break;
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  printf("%ld cases\nok\n", ncase);
  return 0;
}

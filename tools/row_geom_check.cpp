// Walks row_geom (mr-gnas_amd/csrc/row_geom.hpp) over D = 1 .. 1100 with aligned and unaligned bases and checks it against the ten
// <VEC, LPR, KMAX> instances that MRG_DISPATCH_GEOM builds of every row-streaming kernel.  The (width, placement) pairs given
// on the command line -- "64" aligned base, "200u" a base 4 bytes past a 16-byte boundary -- are the widths the GPU matrix runs
// (tests/rowgeom_ref.py) and "!1028" a width that matrix expects to be refused: each is printed with its class, and the program
// fails unless they reach all ten classes, the three-live-step and the four-live-step case of both KMAX = 4 classes, and the
// first refused width of each placement (1028 aligned, 257 scalar, 260 on an unaligned base).  Host code only:
//   c++ -std=c++17 -O1 -I mr-gnas_amd/csrc tools/row_geom_check.cpp -o row_geom_check && ./row_geom_check 4 64 ... 16u ... !1028 !257 !260u
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "row_geom.hpp"

using namespace mrg;

struct Class { const char* name; int vec, lpr, kmax; long walked; int listed; };
static Class classes[] = {
    {"A16", 4, 16, 1, 0, 0}, {"A32", 4, 32, 1, 0, 0}, {"A64k1", 4, 64, 1, 0, 0}, {"A64k2", 4, 64, 2, 0, 0}, {"A64k4", 4, 64, 4, 0, 0},
    {"S16", 1, 16, 1, 0, 0}, {"S32", 1, 32, 1, 0, 0}, {"S64k1", 1, 64, 1, 0, 0}, {"S64k2", 1, 64, 2, 0, 0}, {"S64k4", 1, 64, 4, 0, 0},
};
static const int NCLASS = (int)(sizeof(classes) / sizeof(classes[0]));

static Class* class_of(const RowGeom& g) {
  for (Class& c : classes)
    if (c.vec == g.vec && c.lpr == g.lpr && c.kmax == g.kmax) return &c;
  return nullptr;
}

// live steps of a row: ceil(D / VEC / LPR)
static int live_steps(int D, const RowGeom& g) { return (D / g.vec + g.lpr - 1) / g.lpr; }

int main(int argc, char** argv) {
  int bad = 0;
  // every width: an ok geometry is one of the ten instances and covers the row; the refusals start where the table says
  int first_refused[2] = {0, 0}, first_refused_mult4[2] = {0, 0};
  for (int D = 1; D <= 1100; ++D)
    for (int un = 0; un < 2; ++un) {
      const RowGeom g = row_geom(D, !un);
      if (!g.ok) {
        if (!first_refused[un]) first_refused[un] = D;
        if (D % 4 == 0 && !first_refused_mult4[un]) first_refused_mult4[un] = D;
        continue;
      }
      Class* c = class_of(g);
      if (c == nullptr || g.lpr * g.kmax * g.vec < D || (g.vec == 4 && (D % 4 != 0 || un)) || first_refused_mult4[un]
          || (D % 4 != 0 && first_refused[un])) {
        if (bad++ < 20) printf("bad geometry: D %d unaligned %d -> vec %d lpr %d kmax %d\n", D, un, g.vec, g.lpr, g.kmax);
        continue;
      }
      ++c->walked;
    }
  if (first_refused[0] != 257 || first_refused_mult4[0] != 1028 || first_refused[1] != 257 || first_refused_mult4[1] != 260) {
    printf("refusal edges moved: aligned %d / %d, unaligned %d / %d\n", first_refused[0], first_refused_mult4[0], first_refused[1], first_refused_mult4[1]);
    ++bad;
  }

  // the listed widths
  bool live3[2] = {false, false}, live4[2] = {false, false};       // [0] A64k4, [1] S64k4
  bool edge[3] = {false, false, false};                            // 1028 aligned, 257 scalar, 260 on an unaligned base
  for (int i = 1; i < argc; ++i) {
    const size_t n = strlen(argv[i]);
    const bool un = n > 0 && argv[i][n - 1] == 'u', refuse = argv[i][0] == '!';
    const int D = atoi(argv[i] + (refuse ? 1 : 0));
    const RowGeom g = row_geom(D, !un);
    if (refuse) {
      printf("%s: %s\n", argv[i], g.ok ? "NOT refused" : "refused");
      if (g.ok) ++bad;
      if (!un && D == first_refused_mult4[0]) edge[0] = true;
      if (!un && D == first_refused[0]) edge[1] = true;
      if (un && D == first_refused_mult4[1]) edge[2] = true;
      continue;
    }
    Class* c = g.ok ? class_of(g) : nullptr;
    if (c == nullptr) {
      printf("%s: refused\n", argv[i]);
      ++bad;
      continue;
    }
    const int live = live_steps(D, g);
    printf("%s: %s live %d\n", argv[i], c->name, live);
    ++c->listed;
    if (g.kmax == 4 && live == 3) live3[g.vec == 1] = true;
    if (g.kmax == 4 && live == 4) live4[g.vec == 1] = true;
  }
  int unreached = 0;
  for (const Class& c : classes) {
    printf("%s <%d, %d, %d>: %ld walked, %d listed\n", c.name, c.vec, c.lpr, c.kmax, c.walked, c.listed);
    if (c.walked == 0 || c.listed == 0) ++unreached;
  }
  const int live_missing = !live3[0] + !live4[0] + !live3[1] + !live4[1];
  const int edges_missing = !edge[0] + !edge[1] + !edge[2];
  printf("%d classes, %d never reached, %d live-step cases missing, %d refusal edges missing, %d bad geometries\n", NCLASS, unreached, live_missing,
         edges_missing, bad);
  return unreached == 0 && live_missing == 0 && edges_missing == 0 && bad == 0 ? 0 : 1;
}

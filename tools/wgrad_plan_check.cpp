// Walks the exact-f32 weight-gradient plan (mr-gnas_amd/csrc/wgrad_plan.hpp) over every shape and checks it against the list
// of kernel instances that wgrad.hip builds: an ok plan must land on a listed instance, and every listed instance must be
// reached by some shape.  Host code only:
//   c++ -std=c++17 -O1 -I mr-gnas_amd/csrc tools/wgrad_plan_check.cpp -o wgrad_plan_check && ./wgrad_plan_check
#include <stdio.h>
#include "wgrad_plan.hpp"

using namespace mrg;

struct Inst { bool dma; int tpw, npf; long hits; };
static Inst insts[] = {
#define MRG_DMA_ROW(T, F) {true, T, F, 0},
#define MRG_PLAIN_ROW(T, F) {false, T, F, 0},
    MRG_WGRAD_DMA_INSTANCES(MRG_DMA_ROW) MRG_WGRAD_PLAIN_INSTANCES(MRG_PLAIN_ROW)
};

static int missing = 0;
static void visit(int K, int Nout, bool dma) {
  const WgradPlan p = wgrad_plan(1000, K, Nout, dma);
  if (!p.ok) return;
  const int f = wgrad_npf_class(p.npf);
  if (!wgrad_has_instance(dma, p.tpw, f)) {
    if (missing++ < 20) printf("no instance: dma %d Nout %d K %d -> tpw %d npf %d (class %d)\n", (int)dma, Nout, K, p.tpw, p.npf, f);
    return;
  }
  for (Inst& i : insts)
    if (i.dma == dma && i.tpw == p.tpw && i.npf == f) ++i.hits;
}

int main() {
  for (int Nout = 1; Nout <= 1024; ++Nout)
    for (int K = 1; K <= 4096; ++K) visit(K, Nout, false);
  for (int Nout = 4; Nout <= 224; Nout += 4)            // what the DMA form takes: 16-byte rows of at most seven row tiles
    for (int K = 4; K <= 4096; K += 4) visit(K, Nout, true);
  int unreached = 0;
  for (const Inst& i : insts) {
    printf("%s<%d, %d>: %ld shapes\n", i.dma ? "wgrad_dma_k" : "wgrad_k", i.tpw, i.npf, i.hits);
    if (i.hits == 0) ++unreached;
  }
  printf("%d instances, %d shapes without an instance, %d instances never reached\n", (int)(sizeof(insts) / sizeof(insts[0])), missing, unreached);
  return missing == 0 && unreached == 0 ? 0 : 1;
}

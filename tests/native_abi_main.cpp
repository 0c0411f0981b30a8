// A stand-alone caller of libbeekern.so's pure host entry points, for
// tests/test_native_abi_cpu.py (which compiles it against the built library
// and reads its output): the size of every workspace kind, of the kinds just
// outside the enum, and what bk_workspace_init answers to arguments it must
// refuse before any HIP call.  Needs no GPU.
#include <cstdio>

#include "../csrc/kernels/beekern.h"

int main() {
  printf("count %d\n", (int)BK_WS_COUNT);
  for (int kind = -1; kind <= BK_WS_COUNT; ++kind) printf("bytes %d %lld\n", kind, (long long)bk_workspace_bytes(kind));
  char block[64];
  printf("init %d %d\n", -1, bk_workspace_init(-1, block, nullptr));
  printf("init %d %d\n", (int)BK_WS_COUNT, bk_workspace_init(BK_WS_COUNT, block, nullptr));
  printf("init_null %d\n", bk_workspace_init(BK_WS_REDUCE, nullptr, nullptr));
  return 0;
}

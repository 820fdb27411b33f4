// Host driver of the kernel dispatch (bocf_amd/csrc/kern_dispatch.h) for tests/test_kern_dispatch_cpu.py.
//   kern_dispatch_driver dispatch        for d = 0 ... 33 and kernel id = 0 ... 3 one line "d id D family" with the constants the generic
//                                        lambda was instantiated with, or "d id none" when bocf_dispatch_d did not call it
//   kern_dispatch_driver runs ID [K...]  the (j0, m_run, id) triples of bocf_family_runs, one per line: the list K of per-output ids, or
//                                        with "null M" in its place no list and M outputs of kernel id ID
#include "../bocf_amd/csrc/kern_dispatch.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "dispatch")) {
    for (int d = 0; d <= BOCF_MAX_D + 1; ++d)
      for (int id = 0; id <= 3; ++id) {
        int calls = 0;
        const bool did = bocf_dispatch_d(d, [&](auto Dc) {
          bocf_dispatch_family(id, [&](auto Kc) {
            constexpr int D = decltype(Dc)::value, KID = decltype(Kc)::value;
            static_assert(D >= 1 && D <= BOCF_MAX_D && (KID == 0 || KID == 2 || KID == 3), "instantiated outside the kernels' range");
            printf("%d %d %d %d\n", d, id, D, KID);
            ++calls;
          });
        });
        if (!did) printf("%d %d none\n", d, id);
        if (calls != (did ? 1 : 0)) return fprintf(stderr, "d=%d id=%d: %d calls, returned %d\n", d, id, calls, (int)did), 1;
      }
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "runs")) {
    const int id = atoi(argv[2]);
    std::vector<int> kids;
    int m = 0;
    const bool null_list = argc == 5 && !strcmp(argv[3], "null");
    if (null_list) m = atoi(argv[4]);
    else {
      for (int i = 3; i < argc; ++i) kids.push_back(atoi(argv[i]));
      m = (int)kids.size();
    }
    bocf_family_runs(id, null_list ? nullptr : kids.data(), m, [](int j0, int mr, int kid) { printf("%d %d %d\n", j0, mr, kid); });
    return 0;
  }
  return fprintf(stderr, "usage: kern_dispatch_driver dispatch | runs ID (null M | K...)\n"), 2;
}

// Evaluates the contact kernel's launch planner (csrc/contact_plan.hpp) on the host; driven by tests/test_contact_plan.py.
//   stdin, one case per line: L nq variant rule jpoly split ring_rows waves_per_block queue_slack spec two_wave_vgprs
//   stdout, one line per case: rc family waves_per_pair ring_rows queue_entries lds_bytes_per_wave specialised [| message]
//   (the fields of shpair_get_kernel_info, through contact_kernel_info; all -1 when the planner refuses the shape)
// With the argument "specs" and the two-wave VGPRs of L = 12: "L nq rr qc wpp | rr qc wpp" of every PairSpec<L>, then
// what the planner picks at that shape with the default options.
#include <cstdio>
#include <cstring>

#include "contact_plan.hpp"

using namespace shp;

template <int L>
static void spec_line(const int vgprs)
{
  typedef PairSpec<L> S;
  ContactPlan p;
  const int rc = plan_contact(L, S::nq, ContactOptions{}, vgprs, p);
  printf("%d %d %d %d %d | %d %d %d %d\n", L, S::nq, S::rr, S::qc, S::wpp, rc, p.ring_rows, p.qcap, p.waves_per_pair);
}

int main(int argc, char** argv)
{
  if (argc > 2 && !strcmp(argv[1], "specs")) {
    int v12 = 0;
    sscanf(argv[2], "%d", &v12);
    spec_line<4>(0);
    spec_line<6>(0);
    spec_line<12>(v12);
    return 0;
  }
  int L, nq, vgprs;
  ContactOptions o;
  while (scanf("%d %d %d %d %d %d %d %d %d %d %d", &L, &nq, &o.variant, &o.rule, &o.jpoly, &o.split, &o.ring_rows,
               &o.waves_per_block, &o.queue_slack, &o.spec, &vgprs) == 11) {
    ContactPlan p;
    char msg[256] = "";
    const int rc = plan_contact(L, nq, o, vgprs, p, msg, (int)sizeof(msg));
    shpair_kernel_info k;
    if (rc) {
      printf("%d -1 -1 -1 -1 -1 -1 | %s\n", rc, msg);
      continue;
    }
    contact_kernel_info(p, 0, k);
    printf("%d %d %d %d %d %d %d\n", rc, k.family, k.waves_per_pair, k.ring_rows, k.queue_entries, k.lds_bytes_per_wave,
             k.specialised);
  }
  return 0;
}

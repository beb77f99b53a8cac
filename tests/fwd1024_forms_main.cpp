// Host program of tests/test_fwd1024_forms_cpu.py: the choice of csrc/fwd1024_forms.h without a GPU.
//   fwd1024_forms --forms            one line per form: id, name and the members the test reads
//   fwd1024_forms N:l0,l1,.. ...     the bank shapes (n_filters:pass lengths); calls as records of 16 int16 on stdin, in the
//                                    order of `Record`; prints the form id chosen for each (-1: rejected)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "fwd1024_forms.h"

using namespace at_hip;

struct Bank { int n_filters; std::vector<int> pass_len; };
struct Record {
  short hop, spectrum, phase, polar, channel_major, bank /* index, -1: none */, contrast, power2, out_aligned_512, feat_aligned_16,
      epilogue, dev_stores, dev_persistent, dev_register_tables, dev_no_register_tables, unused;
};

template <class Form> static void print_form(int id, const char* name) {
  printf("%d %s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %llu\n", id, name, id < kFwd1024ProductForms, Form::hop_slots,
         Form::write_phase, Form::polar, Form::mel, Form::window_passes, Form::hoisted_passes, Form::fixed_quads0, Form::fixed_quads1,
         Form::fixed_contrast, Form::fixed_power2, Form::aligned_stores, Form::nontemporal, Form::persistent, Form::packed_passes,
         (unsigned long long)Form::packed_quads);
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--forms")) {
#define X(F) print_form<fwd1024::F>(kFwd##F, #F);
    AT_FWD1024_FORMS(X) AT_FWD1024_DEV_FORMS(X)
#undef X
    return 0;
  }
  std::vector<Bank> banks;
  for (int i = 1; i < argc; ++i) {
    Bank b;
    b.n_filters = atoi(argv[i]);
    const char* s = strchr(argv[i], ':');
    while (s && s[1]) {
      b.pass_len.push_back(atoi(s + 1));
      s = strchr(s + 1, ',');
    }
    banks.push_back(b);
  }
  Record r;
  while (fread(&r, sizeof r, 1, stdin) == 1) {
    Fwd1024Call c = {};
    c.hop = r.hop; c.spectrum = r.spectrum; c.phase = r.phase; c.polar = r.polar; c.channel_major = r.channel_major;
    c.bank = r.bank >= 0;
    if (r.bank >= (int)banks.size()) return 2;
    if (c.bank) {
      const Bank& b = banks[r.bank];
      c.n_passes = (int)b.pass_len.size(); c.n_filters = b.n_filters; c.pass_len = b.pass_len.data();
    }
    c.contrast = r.contrast; c.power2 = r.power2; c.out_aligned_512 = r.out_aligned_512; c.feat_aligned_16 = r.feat_aligned_16;
    c.epilogue = r.epilogue; c.dev_stores = r.dev_stores; c.dev_persistent = r.dev_persistent;
    c.dev_register_tables = r.dev_register_tables; c.dev_no_register_tables = r.dev_no_register_tables;
    printf("%d\n", pick_fwd1024(c));
  }
  return 0;
}

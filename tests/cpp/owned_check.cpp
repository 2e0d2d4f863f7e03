// owned_check.cpp -- stand-alone check of csrc/cc4_owned.h (own main; built with the address and undefined-behaviour sanitizers by
// tests/test_owned_cpu.py): the list of a handle's resources with recording releasers in place of the runtime's.  The fields live in a heap block of
// exactly their size, so a write beside a field is the sanitizer's to report.  Exit status 0: all as expected.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../cage_challenge_4_amd/csrc/cc4_owned.h"

struct Released { int kind; void* p; };
static std::vector<Released> g_log;
static void rel_dev(void* p) { g_log.push_back({OWN_DEVICE, p}); }
static void rel_pin(void* p) { g_log.push_back({OWN_PINNED, p}); }
static void rel_ev(void* p) { g_log.push_back({OWN_EVENT, p}); }
static void rel_st(void* p) { g_log.push_back({OWN_STREAM, p}); }

static int g_failures = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++g_failures; } } while (0)

// a handle's fields as the list sees them: typed pointers, an array among them
struct Fields { int* d_a; char* pin; void* ev; void* st; float* ring[3]; int* never; };
static void* tok(uintptr_t v) { return reinterpret_cast<void*>(v); }
template <class T> static void** fld(T** f) { return reinterpret_cast<void**>(f); }
static bool live_is(const OwnedList& o, int64_t d, int64_t p, int64_t e, int64_t s) {
  int64_t n[OWN_KINDS] = {0, 0, 0, 0};
  o.count_live(n);
  return n[OWN_DEVICE] == d && n[OWN_PINNED] == p && n[OWN_EVENT] == e && n[OWN_STREAM] == s;
}

int main() {
  Fields* f = static_cast<Fields*>(malloc(sizeof(Fields)));
  memset(f, 0, sizeof(Fields));
  OwnedList o{{rel_dev, rel_pin, rel_ev, rel_st}, {}};

  // registration: all four kinds, two elements of an array, one field never filled; a field registered twice is one entry
  o.add(fld(&f->st), OWN_STREAM);   f->st = tok(0x40);
  o.add(fld(&f->d_a), OWN_DEVICE);  f->d_a = static_cast<int*>(tok(0x10));
  o.add(fld(&f->pin), OWN_PINNED);  f->pin = static_cast<char*>(tok(0x20));
  o.add(fld(&f->ev), OWN_EVENT);    f->ev = tok(0x30);
  o.add(fld(&f->ring[0]), OWN_DEVICE); f->ring[0] = static_cast<float*>(tok(0x50));
  o.add(fld(&f->ring[2]), OWN_DEVICE); f->ring[2] = static_cast<float*>(tok(0x52));
  o.add(fld(&f->never), OWN_DEVICE);
  EXPECT(o.entries.size() == 7);
  o.add(fld(&f->d_a), OWN_DEVICE);
  o.add(fld(&f->ring[2]), OWN_DEVICE);
  EXPECT(o.entries.size() == 7);
  EXPECT(live_is(o, 3, 1, 1, 1));
  EXPECT(g_log.empty());

  // one field now: its releaser once with the old value, the field null, the count down by one, the entry kept
  o.release(fld(&f->d_a));
  EXPECT(g_log.size() == 1 && g_log[0].kind == OWN_DEVICE && g_log[0].p == tok(0x10));
  EXPECT(f->d_a == nullptr && o.entries.size() == 7);
  EXPECT(live_is(o, 2, 1, 1, 1));
  o.release(fld(&f->d_a));                        // nothing in it: nothing called
  o.release(fld(&f->never));
  o.release(fld(&f->ring[1]));                    // not a field of the list's: nothing called, nothing written
  EXPECT(g_log.size() == 1 && f->ring[1] == nullptr);
  // filled again (the free-and-reallocate sites): counted again
  f->d_a = static_cast<int*>(tok(0x11));
  EXPECT(live_is(o, 3, 1, 1, 1));

  // everything: each non-null field exactly once, last registered first, every field null afterwards
  g_log.clear();
  o.release_all();
  const Released want[] = {{OWN_DEVICE, tok(0x52)}, {OWN_DEVICE, tok(0x50)}, {OWN_EVENT, tok(0x30)}, {OWN_PINNED, tok(0x20)}, {OWN_DEVICE, tok(0x11)}, {OWN_STREAM, tok(0x40)}};
  EXPECT(g_log.size() == 6);
  for (size_t i = 0; i < 6 && i < g_log.size(); ++i) EXPECT(g_log[i].kind == want[i].kind && g_log[i].p == want[i].p);
  EXPECT(!f->d_a && !f->pin && !f->ev && !f->st && !f->ring[0] && !f->ring[1] && !f->ring[2] && !f->never);
  EXPECT(live_is(o, 0, 0, 0, 0));
  o.release_all();                                // a second time: nothing called
  EXPECT(g_log.size() == 6);

  free(f);
  printf("owned_check: %d failures\n", g_failures);
  return g_failures ? 1 : 0;
}

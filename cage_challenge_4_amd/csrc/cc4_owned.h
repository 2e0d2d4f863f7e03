// cc4_owned.h -- who frees what a handle allocates: a list of (address of the owning field, kind).  The field stays the raw pointer everybody reads; the
// list knows where it lives and how to give back what it points to.  No HIP in here: the releasers come in as function pointers (cc4_host.h passes
// hipFree, hipHostFree, hipEventDestroy and hipStreamDestroy; tests/cpp/owned_check.cpp passes recorders).
#pragma once
#include <stdint.h>
#include <vector>

enum OwnedKind { OWN_DEVICE = 0, OWN_PINNED = 1, OWN_EVENT = 2, OWN_STREAM = 3, OWN_KINDS = 4 };
struct OwnedList {
  struct Entry { void** field; OwnedKind kind; };
  void (*releaser[OWN_KINDS])(void*);
  std::vector<Entry> entries;                    // in order of registration
  // the field is the list's from now on (again for a field it already has: nothing).  An element of an array is a field of its own.
  void add(void** field, OwnedKind kind) {
    for (const Entry& e : entries) if (e.field == field) return;
    entries.push_back(Entry{field, kind});
  }
  // what the field points to goes back now; the field is null afterwards and stays registered, for the next allocation into it
  void release(void** field) {
    for (const Entry& e : entries) if (e.field == field && *field) { void* const p = *field; *field = nullptr; releaser[e.kind](p); }
  }
  // everything, last registered first
  void release_all() { for (size_t i = entries.size(); i-- > 0;) release(entries[i].field); }
  // fields that hold something, per kind: ADDED to out
  void count_live(int64_t out[OWN_KINDS]) const { for (const Entry& e : entries) if (*e.field) ++out[e.kind]; }
};

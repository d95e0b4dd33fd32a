// own_check.cpp -- lbm_own::Own (lbm-asynchronous_amd/csrc/lbm_own.h) with a counting release function, as a stand-alone
// program: exit status 0 when the handle releases what it owns exactly once and in the order Slab relies on, else 1 and
// the failed checks on stderr.  tests/test_own_handle.py builds it under AddressSanitizer and UBSan and runs it.
#include "../lbm-asynchronous_amd/csrc/lbm_own.h"

#include <cstdio>
#include <type_traits>
#include <utility>
#include <vector>

namespace {

std::vector<int> g_released;  // every value handed to the release function, in order
void count_release(int v) { g_released.push_back(v); }
using Handle = lbm_own::Own<int, count_release>;  // 0 is the empty value

int* g_freed = nullptr;  // a pointer instance: what the device buffers are
void free_int(int* p) { g_freed = p; delete p; }
using IntPtr = lbm_own::Own<int*, free_int>;

static_assert(!std::is_copy_constructible<Handle>::value && !std::is_copy_assignable<Handle>::value, "move-only");
static_assert(std::is_nothrow_move_constructible<Handle>::value && std::is_nothrow_move_assignable<Handle>::value, "movable");

int g_failures = 0;
void check(bool ok, const char* what) {
  if (!ok) { fprintf(stderr, "own_check: FAILED: %s\n", what); g_failures++; }
}
bool released_is(std::initializer_list<int> want) { return g_released == std::vector<int>(want); }

struct Body {  // what Slab relies on: the destructor's body first, then the members in reverse order of declaration
  Handle first{1}, second{2}, third{3};
  ~Body() { g_released.push_back(-1); second.reset(); }
};

}  // namespace

int main() {
  {
    Handle h;
    check(!h && h.get() == 0, "a default handle is empty");
    h.reset();
  }
  check(released_is({}), "an empty handle releases nothing (scope end, reset)");

  {
    Handle h(7);
    check(h && h.get() == 7, "a full handle holds its value");
    const int raw = h;  // the implicit conversion
    check(raw == 7 && released_is({}), "reading the value releases nothing");
  }
  check(released_is({7}), "a full handle releases exactly once at scope end");

  g_released.clear();
  {
    Handle h(8);
    h.reset();
    check(released_is({8}) && !h && h.get() == 0, "reset() releases once and leaves the handle empty");
    h.reset(9);
    check(released_is({8}) && h.get() == 9, "reset(v) on an empty handle releases nothing and holds v");
    h.reset(10);
    check(released_is({8, 9}) && h.get() == 10, "reset(v) on a full handle releases the old value");
  }
  check(released_is({8, 9, 10}), "... and the last value once at scope end");

  g_released.clear();
  {
    Handle h(11);
    const int out = h.release();
    check(out == 11 && !h, "release() hands the value out and leaves the handle empty");
  }
  check(released_is({}), "release() releases nothing, nor does the handle afterwards");

  {
    Handle a(12);
    Handle b(std::move(a));
    check(!a && a.get() == 0 && b.get() == 12 && released_is({}), "a moved-from handle is empty, nothing released by the move");
  }
  check(released_is({12}), "the target of a move construction releases once");

  g_released.clear();
  {
    Handle a(13), b(14);
    b = std::move(a);
    check(released_is({14}) && !a && b.get() == 13, "move assignment onto a full handle releases the old value first, once");
  }
  check(released_is({14, 13}), "... and the moved value once at scope end");

  g_released.clear();
  {
    Handle a(15);
    Handle& alias = a;
    a = std::move(alias);
    check(released_is({}) && a.get() == 15, "self-move-assignment does not release");
  }
  check(released_is({15}), "... and the value goes once at scope end");

  g_released.clear();
  { Body b; }
  check(released_is({-1, 2, 3, 1}), "a struct's members go in reverse declaration order, after its destructor's body");

  {
    IntPtr p(new int(5));
    check(p && *p == 5 && p[0] == 5 && p + 0 == p.get(), "a pointer handle reads as the pointer");
    int* const raw = p.get();
    IntPtr q;
    q = std::move(p);
    check(!p && q.get() == raw && g_freed == nullptr, "moving a pointer handle frees nothing");
    q.reset();
    check(g_freed == raw && !q, "reset() frees the pointer");
  }

  if (g_failures == 0) printf("own_check: ok\n");
  return g_failures == 0 ? 0 : 1;
}

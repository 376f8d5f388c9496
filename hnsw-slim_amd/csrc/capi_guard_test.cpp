// capi_guard_test.cpp -- host-only test of csrc/capi_guard.hpp, built with AddressSanitizer and UBSan (Makefile target
// capi_guard_test): what a body that throws comes out as -- the statuses and texts the C ABI's hand-written handlers gave before the
// guard replaced them --, that a returned status passes through with the error text untouched, and the scope guard.
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "capi_guard.hpp"

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("FAILED line %d: %s (text \"%s\")\n", __LINE__, #cond, g_err.c_str()); \
      failures++;                                                     \
    }                                                                 \
  } while (0)

template <class E>
static hs_status thrown(const E &e) {
  return guarded([&]() -> hs_status { throw e; });
}
static bool text_is(const char *t) { return g_err == t; }

int main() {
  // std::bad_alloc: the default text and an entry's own
  CHECK(thrown(std::bad_alloc()) == HS_ERR_NOMEM && text_is("Not enough memory"));
  CHECK(guarded("Not enough memory: addPoint failed to allocate linklist", []() -> hs_status { throw std::bad_alloc(); }) == HS_ERR_NOMEM &&
        text_is("Not enough memory: addPoint failed to allocate linklist"));
  // from_exception's mapping, text kept
  CHECK(thrown(std::runtime_error("Cannot open file")) == HS_ERR_IO && text_is("Cannot open file"));
  CHECK(thrown(std::runtime_error("Index seems to be corrupted or unsupported")) == HS_ERR_CORRUPT && text_is("Index seems to be corrupted or unsupported"));
  CHECK(thrown(std::runtime_error("Not enough memory: loadIndex failed to allocate level0")) == HS_ERR_NOMEM &&
        text_is("Not enough memory: loadIndex failed to allocate level0"));
  CHECK(thrown(std::runtime_error("brute force supports dim <= 4096")) == HS_ERR_UNSUPPORTED && text_is("brute force supports dim <= 4096"));
  CHECK(thrown(std::runtime_error("SlimQ supports 64 <= dim < 4096")) == HS_ERR_UNSUPPORTED);
  CHECK(thrown(std::runtime_error("Label not found")) == HS_ERR_INVALID && text_is("Label not found"));
  CHECK(thrown(std::length_error("anything else")) == HS_ERR_INVALID && text_is("anything else"));
  // an entry with texts of its own maps first and falls back
  auto own = [](const std::exception &e) { return std::strcmp(e.what(), "full") == 0 ? fail(HS_ERR_CAPACITY, e.what()) : from_exception(e); };
  CHECK(guarded("Not enough memory", []() -> hs_status { throw std::runtime_error("full"); }, own) == HS_ERR_CAPACITY && text_is("full"));
  CHECK(guarded("Not enough memory", []() -> hs_status { throw std::runtime_error("Cannot open file"); }, own) == HS_ERR_IO);
  CHECK(guarded("own text", []() -> hs_status { throw std::bad_alloc(); }, own) == HS_ERR_NOMEM && text_is("own text"));
  // not a std::exception
  CHECK(thrown(7) == HS_ERR_INVALID && text_is("unknown exception"));
  // a returned status passes through, the text untouched
  fail(HS_ERR_INVALID, "earlier");
  CHECK(guarded([] { return HS_OK; }) == HS_OK && text_is("earlier"));
  CHECK(guarded([] { return HS_ERR_CAPACITY; }) == HS_ERR_CAPACITY && text_is("earlier"));
  CHECK(guarded("x", [] { return fail(HS_ERR_DEVICE, "its own") ; }) == HS_ERR_DEVICE && text_is("its own"));
  CHECK(fail(HS_ERR_IO, std::string("built ") + "text") == HS_ERR_IO && text_is("built text"));

  // the scope guard: on return, on throw; dismissed, not at all
  int ran = 0;
  {
    const Restore r([&] { ran++; });
  }
  CHECK(ran == 1);
  CHECK(guarded([&]() -> hs_status {
          const Restore r([&] { ran++; });
          throw std::runtime_error("Cannot open file");
        }) == HS_ERR_IO);
  CHECK(ran == 2);
  auto only_on_failure = [&](bool ok) {
    return guarded([&]() -> hs_status {
      Restore undo([&] { ran += 10; });
      if (!ok) throw std::bad_alloc();
      undo.dismiss();
      return HS_OK;
    });
  };
  CHECK(only_on_failure(true) == HS_OK && ran == 2);
  CHECK(only_on_failure(false) == HS_ERR_NOMEM && ran == 12);
  {   // a refusal by return, not by throw, un-dismissed: undone as well
    Restore undo([&] { ran += 100; });
  }
  CHECK(ran == 112);

  if (failures) return 1;
  printf("capi_guard ok\n");
  return 0;
}

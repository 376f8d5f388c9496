// capi_guard.hpp -- how the C ABI reports: the calling thread's error text (hs_last_error), the mapping of an exception's text to a
// status, the guard every exported entry that can throw runs its body in (no exception leaves an extern "C" function), and a scope
// guard for the state an entry must put back.  No HIP here: csrc/capi_guard_test.cpp builds it alone.
#pragma once
#include <exception>
#include <new>
#include <string>
#include <utility>

#include "../../include/hnsw_slim_amd.h"

#pragma GCC visibility push(hidden)
inline thread_local std::string g_err;   // hs_last_error

inline hs_status fail(hs_status s, const std::string &msg) {
  g_err = msg;
  return s;
}
// (a literal: nothing is built on the way in, and a text that cannot be stored is dropped -- the handlers below call this one)
inline hs_status fail(hs_status s, const char *msg) noexcept {
  try {
    g_err.assign(msg);
  } catch (...) {
    g_err.clear();
  }
  return s;
}
// the reference's exception texts with the statuses the header documents
inline hs_status from_exception(const std::exception &e) {
  std::string m = e.what();
  if (m == "Cannot open file") return fail(HS_ERR_IO, m);
  if (m.find("corrupted") != std::string::npos) return fail(HS_ERR_CORRUPT, m);
  if (m.find("Not enough memory") != std::string::npos) return fail(HS_ERR_NOMEM, m);
  if (m.find("supports dim") != std::string::npos || m.find("SlimQ supports") != std::string::npos) return fail(HS_ERR_UNSUPPORTED, m);
  return fail(HS_ERR_INVALID, m);
}

// body() returns an hs_status; what it throws becomes one.  on_exception maps a std::exception (from_exception unless the entry has
// texts of its own).  A plain template, so the body inlines: a try region costs nothing until something throws.
template <class F, class M>
hs_status guarded(const char *nomem_text, F &&body, M &&on_exception) {
  try {
    return body();
  } catch (std::bad_alloc &) {
    return fail(HS_ERR_NOMEM, nomem_text);
  } catch (std::exception &e) {
    try {
      return on_exception(e);
    } catch (...) {   // (the text could not be copied)
      return fail(HS_ERR_NOMEM, nomem_text);
    }
  } catch (...) {
    return fail(HS_ERR_INVALID, "unknown exception");
  }
}
template <class F>
hs_status guarded(const char *nomem_text, F &&body) {
  return guarded(nomem_text, std::forward<F>(body), from_exception);
}
template <class F>
hs_status guarded(F &&body) {
  return guarded("Not enough memory", std::forward<F>(body), from_exception);
}

// Runs `undo` when the scope ends, by return or by exception, unless dismiss() was called: what a success keeps, it dismisses.
template <class F>
struct Restore {
  F undo;
  bool armed = true;
  explicit Restore(F f) : undo(std::move(f)) {}
  Restore(const Restore &) = delete;
  Restore &operator=(const Restore &) = delete;
  void dismiss() { armed = false; }
  ~Restore() {
    if (armed) undo();
  }
};
#pragma GCC visibility pop

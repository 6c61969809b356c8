#pragma once
// The C ABI of the native libraries, written once: every exported function is defined with
// TTDK_API / TTD_API, which records "name ret:args" — one letter per type, computed from the
// function's own type — in a table the library exports (TTD_ABI_TABLE). Python sets its ctypes
// argtypes / restype from that table (ops/_lib.py), so a signature exists in one place only.
// Host-only, no HIP headers.
//
//   v void (return only)   i int     u unsigned   l long / long long   Q unsigned long (long)
//   f float   d double     P any pointer (hipStream_t included)        z const char* return
//   E const TtdkEpilogue*  G const TtdkConv*      D const TtdkDwConv*  (next to each struct)
//
// Code has no primary definition: an export taking any other type (bool, short, a struct by
// value) does not compile.
#include <cstddef>
#include <cstring>

namespace ttd_abi {

template <class T>
struct Code;
#define TTD_ABI_CODE(TYPE, LETTER) \
  template <>                      \
  struct Code<TYPE> {              \
    static constexpr char code = LETTER; \
  }
TTD_ABI_CODE(void, 'v');
TTD_ABI_CODE(int, 'i');
TTD_ABI_CODE(unsigned, 'u');
TTD_ABI_CODE(long, 'l');
TTD_ABI_CODE(long long, 'l');
TTD_ABI_CODE(unsigned long, 'Q');
TTD_ABI_CODE(unsigned long long, 'Q');
TTD_ABI_CODE(float, 'f');
TTD_ABI_CODE(double, 'd');
static_assert(sizeof(long) == 8, "'l' and 'Q' stand for 64-bit integers");
template <class T>
struct Code<T*> {
  static constexpr char code = 'P';
};

template <class R>
struct Ret : Code<R> {};
template <>
struct Ret<const char*> {
  static constexpr char code = 'z';
};

// One exported function. The objects are namespace-scope statics of the translation unit that
// defines the function; they link themselves into a list whose head is a function-local static
// (hidden visibility: one list per shared object), so there is no heap and no dependence on the
// order in which translation units initialise.
struct Entry {
  char text[96];  // "name ret:args"
  const Entry* next;

  template <size_t N, class R, class... A>
  Entry(const char (&name)[N], R (*)(A...)) : next(head()) {
    const char sig[] = {' ', Ret<R>::code, ':', Code<A>::code..., '\0'};
    static_assert(N - 1 + sizeof(sig) <= sizeof(text), "name and signature must fit in Entry::text");
    std::memcpy(text, name, N - 1);
    std::memcpy(text + N - 1, sig, sizeof(sig));
    head() = this;
  }
  static const Entry*& head() {
    static const Entry* h = nullptr;
    return h;
  }
};

inline int count() {
  int n = 0;
  for (const Entry* e = Entry::head(); e; e = e->next) ++n;
  return n;
}
inline const char* entry(int i) {
  for (const Entry* e = Entry::head(); e; e = e->next)
    if (i-- == 0) return e->text;
  return nullptr;
}

}  // namespace ttd_abi

// Definition header of an exported function: TTDK_API(int, ttdk_f, (int a, float* b)) { ... }
#define TTD_ABI_EXPORT extern "C" __attribute__((visibility("default")))
#define TTD_API(RET, NAME, ARGS)                                    \
  TTD_ABI_EXPORT RET NAME ARGS;                                     \
  static const ::ttd_abi::Entry ttd_abi_entry_##NAME{#NAME, &NAME}; \
  TTD_ABI_EXPORT RET NAME ARGS
#define TTDK_API TTD_API

// Once per library: PREFIX_count() and PREFIX_entry(i) -> "name ret:args" (null past the end).
#define TTD_ABI_TABLE(PREFIX)                                          \
  TTD_API(int, PREFIX##_count, ()) { return ::ttd_abi::count(); }      \
  TTD_API(const char*, PREFIX##_entry, (int i)) { return ::ttd_abi::entry(i); }

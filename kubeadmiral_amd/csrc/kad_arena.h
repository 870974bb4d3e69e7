// The staging arena of a consumer call: one device buffer laid out from 256-B aligned parts, inputs copied
// from the host and outputs the kernels write. The layout half needs no HIP (KAD_HOST_ONLY stops after it:
// tests/arena_main.cpp); the second half puts a layout on a device buffer.
//   Arena a;  Part x = a.in(host, bytes), y = a.out(bytes);  a.commit(c, buf);  a.ptr<T>(buf, x) ...
#pragma once

#include <cstddef>
#include <vector>

#ifndef KAD_HOST_ONLY
#include "kad_ctx.h"
#endif

struct Part {
  const void* h;     // host source of an input (null: nothing to copy)
  size_t bytes, at;  // at: offset in the buffer; Arena::ABSENT for a part that was declared absent
};

class Arena {
 public:
  static constexpr size_t ALIGN = 256, ABSENT = ~(size_t)0;
  // an input of `bytes` bytes copied from h by commit (h may be null when bytes is 0), with `pad` more bytes
  // reserved behind them for a kernel that may read one element past
  Part in(const void* h, size_t bytes, size_t pad = 0) {
    const Part p = take(h, bytes, pad);
    if (h && bytes) ins_.push_back(p);
    return p;
  }
  Part out(size_t bytes) { return take(nullptr, bytes, 0); }
  // an optional array the caller left out: no slot, and ptr() gives null
  static Part absent() { return Part{nullptr, 0, ABSENT}; }
  size_t total() const { return total_; }
  const std::vector<Part>& inputs() const { return ins_; }

  // the part's address in a buffer that starts at base; null for an absent part
  template <class T>
  static T* ptr(void* base, const Part& p) {
    return p.at == ABSENT ? nullptr : reinterpret_cast<T*>(static_cast<char*>(base) + p.at);
  }

#ifndef KAD_HOST_ONLY
  inline int commit(kad_ctx* c, DevBuf& buf) const;
  template <class T>
  static T* ptr(const DevBuf& buf, const Part& p) { return ptr<T>(buf.p, p); }
#endif

 private:
  // every part starts on a 256-B boundary; an empty one still takes a slot, so no two parts share an address
  Part take(const void* h, size_t bytes, size_t pad) {
    const Part p{h, bytes, total_};
    total_ += bytes + pad ? (bytes + pad + ALIGN - 1) / ALIGN * ALIGN : ALIGN;
    return p;
  }
  size_t total_ = 0;
  std::vector<Part> ins_;
};

#ifndef KAD_HOST_ONLY
// grows buf to the layout (kept when it already holds it) and issues one copy per non-empty input on the
// ctx's stream; the host arrays must stay valid until the stream is synchronised
inline int Arena::commit(kad_ctx* c, DevBuf& buf) const {
  if (int r = grow(c, buf, total_)) return r;
  for (const Part& p : ins_)
    HIPCHK(c, hipMemcpyAsync(buf.as<char>() + p.at, p.h, p.bytes, hipMemcpyHostToDevice, c->stream));
  return 0;
}
#endif  // KAD_HOST_ONLY

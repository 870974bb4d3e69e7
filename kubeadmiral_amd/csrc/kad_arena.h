// The staging arena of a consumer call: one device buffer laid out from 256-B aligned parts, inputs copied
// from the host and outputs the kernels write. Every part is bound to the device pointer it fills, so that its
// width comes from the field's type and its count is in elements. The layout half needs no HIP (KAD_HOST_ONLY
// stops after it: tests/arena_main.cpp); the second half puts a layout on a device buffer.
//   Arena a;  a.in(d.x, host_x, n);  a.out(d.y, host_y, m);  a.out(d.tmp, k);  a.absent(d.z);
//   a.commit(c, buf);  ...launch with d...  a.fetch(c);
#pragma once

#include <cstddef>
#include <cstring>
#include <vector>

#ifndef KAD_HOST_ONLY
#include "kad_ctx.h"
#endif

class Arena {
 public:
  static constexpr size_t ALIGN = 256;
  struct Part {
    void* field;       // the bound device pointer (a T* or const T* object), patched by place()
    const void* h;     // host source of an input (null: nothing to copy)
    void* back;        // host destination of an output (null: it stays on the device)
    size_t bytes, at;  // at: offset in the buffer
  };
  // an input of n elements copied from h by commit (h may be null when n is 0), with `pad` more elements
  // reserved behind them for a kernel that may read past the end
  template <class T>
  void in(const T*& d, const T* h, size_t n, size_t pad = 0) {
    take(&d, h, nullptr, n * sizeof(T), pad * sizeof(T));
  }
  // an output of n elements; fetch copies it to `back` (null, or left out: device-only scratch)
  template <class T>
  void out(T*& d, T* back, size_t n) { take(&d, nullptr, back, n * sizeof(T), 0); }
  template <class T>
  void out(T*& d, size_t n) { take(&d, nullptr, nullptr, n * sizeof(T), 0); }
  // an optional array the caller left out: no slot, a null pointer
  template <class T>
  static void absent(T*& d) { d = nullptr; }

  size_t total() const { return total_; }
  const std::vector<Part>& parts() const { return parts_; }  // in declaration order
  // what commit and fetch copy: the non-empty inputs with a source / outputs with a destination
  static bool copied_in(const Part& p) { return p.h && p.bytes; }
  static bool copied_out(const Part& p) { return p.back && p.bytes; }
  // every bound pointer = base + its part's offset
  void place(void* base) const {
    for (const Part& p : parts_) {
      char* at = static_cast<char*>(base) + p.at;
      std::memcpy(p.field, &at, sizeof at);  // (object pointers share one representation)
    }
  }

#ifndef KAD_HOST_ONLY
  inline int commit(kad_ctx* c, DevBuf& buf) const;
  inline int fetch(kad_ctx* c) const;
#endif

 private:
  // every part starts on a 256-B boundary; an empty one still takes a slot, so no two parts share an address
  void take(void* field, const void* h, void* back, size_t bytes, size_t pad) {
    parts_.push_back(Part{field, h, back, bytes, total_});
    total_ += bytes + pad ? (bytes + pad + ALIGN - 1) / ALIGN * ALIGN : ALIGN;
  }
  size_t total_ = 0;
  std::vector<Part> parts_;
};

#ifndef KAD_HOST_ONLY
// grows buf to the layout (kept when it already holds it), points every bound pointer into it and issues one
// copy per non-empty input on the ctx's stream; the host arrays must stay valid until the stream is synchronised
inline int Arena::commit(kad_ctx* c, DevBuf& buf) const {
  if (int r = grow(c, buf, total_)) return r;
  place(buf.p);
  for (const Part& p : parts_)
    if (copied_in(p))
      HIPCHK(c, hipMemcpyAsync(buf.as<char>() + p.at, p.h, p.bytes, hipMemcpyHostToDevice, c->stream));
  return 0;
}
// one copy per non-empty output bound to a host destination, on the ctx's stream, in declaration order
inline int Arena::fetch(kad_ctx* c) const {
  for (const Part& p : parts_)
    if (copied_out(p)) {
      void* d;
      std::memcpy(&d, p.field, sizeof d);
      HIPCHK(c, hipMemcpyAsync(p.back, d, p.bytes, hipMemcpyDeviceToHost, c->stream));
    }
  return 0;
}
#endif  // KAD_HOST_ONLY

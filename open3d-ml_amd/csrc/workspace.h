// workspace.h — how every op lays out the workspace its caller owns.  Host code only.
//
// A workspace's layout is written ONCE, as a function `X x_ws(WsLayout& L, dimensions...)` that takes the pieces one by one and
// returns them in the op's struct.  The size entry runs it on a measuring walker (ws_bytes_of); the op runs it on a carving walker
// over the caller's buffer (ws_carve) and refuses the buffer when bytes() exceeds what it was given.  Every piece starts on a
// 256-byte boundary.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ml3d {

constexpr size_t WS_ALIGN = 256;
static inline size_t ws_up(size_t x) { return (x + (WS_ALIGN - 1)) & ~(WS_ALIGN - 1); }
// a caller's workspace from its first 256-byte boundary on (null stays null), and what is left of `bytes` whatever the alignment cost
static inline char* ws_align(void* ws) { return (char*)(((uintptr_t)ws + (WS_ALIGN - 1)) & ~(uintptr_t)(WS_ALIGN - 1)); }
static inline size_t ws_avail(const void* ws, size_t bytes) { return ws && bytes > WS_ALIGN ? bytes - WS_ALIGN : 0; }

// bits needed to represent every value in [0, v] (at least 1): the key width handed to the radix sorts
static inline int key_bits_for(uint64_t v) {
    int b = 1;
    while (b < 64 && (v >> b) != 0ull) ++b;
    return b;
}

class WsLayout {
public:
    WsLayout() {}                                   // measuring: every take() is null, bytes() is the need
    WsLayout(void* ws, size_t bytes) : base_(ws_align(ws)) {   // carving; a null `ws` measures
        const size_t lost = (size_t)(base_ - (char*)ws);
        cap_ = ws && bytes > lost ? bytes - lost : 0;
    }
    // the next piece: `count` elements of T, rounded up to the alignment.  Null when measuring or when the piece does not fit;
    // the offset advances either way, so bytes() reports the need of a layout that ran out.
    template <class T> T* take(size_t count) { return (T*)raw(sizeof(T) * count); }
    // a nested region of `bytes` (a GridWs, SortWs or FusedWs inside another workspace): a walker of its own over that region
    WsLayout sub(size_t bytes) {
        char* p = raw(bytes);
        return p ? WsLayout(p, bytes) : WsLayout();
    }
    void pad(size_t bytes) { off_ += bytes; }      // trailing slack, added exactly as given
    size_t bytes() const { return off_ + WS_ALIGN; }   // what a buffer must hold: the pieces plus the cost of aligning any base
    bool fits() const { return base_ && off_ <= cap_; }

private:
    char* raw(size_t bytes) {
        const size_t at = off_;
        off_ += ws_up(bytes);
        return base_ && off_ <= cap_ ? base_ + at : nullptr;
    }
    char* base_ = nullptr;
    size_t cap_ = 0, off_ = 0;
};

// what the layout function `layout(L, a...)` asks for: the body of a size entry
template <class F, class... A> size_t ws_bytes_of(F layout, A... a) {
    WsLayout L;
    layout(L, a...);
    return L.bytes();
}
// the opening of an op: *out = the pieces of that layout in the caller's buffer; false when the buffer is smaller than ws_bytes_of
template <class T, class F, class... A> bool ws_carve(void* ws, size_t bytes, T* out, F layout, A... a) {
    WsLayout L(ws, bytes);
    *out = layout(L, a...);
    return L.bytes() <= bytes;
}
// that layout as a region of its own inside the workspace `L` walks (a grid or the sort's scratch inside another op's workspace)
template <class F, class... A> auto ws_nest(WsLayout& L, F layout, A... a) {
    WsLayout S = L.sub(ws_bytes_of(layout, a...));
    return layout(S, a...);
}

}  // namespace ml3d

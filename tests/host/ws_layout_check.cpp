// Stand-alone check of csrc/workspace.h (host code only): build with -fsanitize=address,undefined and run.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "workspace.h"

using namespace ml3d;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

struct Inner { int* a; double* b; };
struct Outer { char* head; Inner in; float* tail; uint64_t* rest; };

static Inner inner_ws(WsLayout& L, size_t n) {
    Inner o;
    o.a = L.take<int>(n);
    o.b = L.take<double>(n + 2);
    return o;
}
static size_t inner_bytes(size_t n) { return ws_bytes_of(inner_ws, n); }
static Outer outer_ws(WsLayout& L, size_t n) {
    Outer o;
    o.head = L.take<char>(1);
    o.in = ws_nest(L, inner_ws, n);
    o.tail = L.take<float>(3 * n);
    o.rest = L.take<uint64_t>(0);
    L.pad(40);
    return o;
}

int main() {
    CHECK(ws_up(0) == 0 && ws_up(1) == 256 && ws_up(256) == 256 && ws_up(257) == 512);
    for (size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)1000}) {
        // measuring: every piece null, bytes() the need
        WsLayout M;
        const Outer m = outer_ws(M, n);
        CHECK(!M.fits() && !m.head && !m.in.a && !m.in.b && !m.tail && !m.rest);
        const size_t need = M.bytes();
        CHECK(need == ws_bytes_of(outer_ws, n));
        const size_t pieces = 256 + inner_bytes(n) + ws_up(12 * n);
        CHECK(inner_bytes(n) == ws_up(4 * n) + ws_up(8 * (n + 2)) + 256);
        CHECK(need == pieces + 40 + 256);                      // pad() adds exactly what it is given; + the base's alignment slack
        // carving an exact-fit buffer at every misalignment: the same offsets, every piece aligned and inside
        for (size_t shift : {(size_t)0, (size_t)1, (size_t)8, (size_t)255}) {
            std::vector<char> buf(need + shift);                // (exactly `need` bytes from buf + shift on: the sanitizer guards both ends)
            char* ws = buf.data() + shift;
            WsLayout L(ws, need);
            Outer o = outer_ws(L, n);
            CHECK(L.fits() && L.bytes() == need);
            char* base = ws_align(ws);
            CHECK(o.head == base && (char*)o.in.a == base + 256 && (char*)o.in.b == base + 256 + ws_up(4 * n));
            CHECK((char*)o.tail == base + 256 + inner_bytes(n) && (char*)o.rest == base + pieces);
            for (void* p : {(void*)o.head, (void*)o.in.a, (void*)o.in.b, (void*)o.tail, (void*)o.rest}) {
                CHECK(p && ((uintptr_t)p & 255) == 0 && (char*)p >= ws && (char*)p <= ws + need);
            }
            CHECK((char*)o.tail + 12 * n <= ws + need);
            // every byte of every piece is the caller's
            o.head[0] = 1;
            for (size_t i = 0; i < n; ++i) { o.in.a[i] = 1; o.tail[3 * i + 2] = 1.f; }
            for (size_t i = 0; i < n + 2; ++i) o.in.b[i] = 1.0;
            // ws_carve: the op's opening -- exact fit passes and gives the same pieces, one byte less is refused
            Outer c;
            CHECK(ws_carve(ws, need, &c, outer_ws, n) && c.head == o.head && c.in.b == o.in.b && c.tail == o.tail && c.rest == o.rest);
            CHECK(!ws_carve(ws, need - 1, &c, outer_ws, n));
            // exhausted: one piece too many comes back null, later ones too, and bytes() still counts
            WsLayout X(ws, need);
            o = outer_ws(X, n);
            CHECK(X.take<char>(need) == nullptr && X.take<char>(1) == nullptr && !X.fits());
            CHECK(X.bytes() == need + ws_up(need) + 256);
            WsLayout sub_of_exhausted = X.sub(512);
            CHECK(sub_of_exhausted.take<int>(1) == nullptr && sub_of_exhausted.bytes() == 512);
        }
        // the 256 bytes of slack in bytes() cover the worst alignment of the base exactly; a null buffer measures
        WsLayout S((void*)(uintptr_t)0x1001, need - 1);
        outer_ws(S, n);
        CHECK(S.bytes() == need && S.fits());
        WsLayout T((void*)(uintptr_t)0x1001, need - 2);
        outer_ws(T, n);
        CHECK(T.bytes() == need && !T.fits());
        WsLayout N(nullptr, 1 << 20);
        CHECK(!outer_ws(N, n).head && !N.fits() && N.bytes() == need);
    }
    CHECK(ws_align(nullptr) == nullptr && ws_avail(nullptr, 4096) == 0 && ws_avail((void*)8, 256) == 0 && ws_avail((void*)8, 4096) == 3840);
    CHECK(key_bits_for(0) == 1 && key_bits_for(1) == 1);
    for (int k = 1; k < 64; ++k) {
        CHECK(key_bits_for((1ull << k) - 1) == k);
        CHECK(key_bits_for(1ull << k) == k + 1);
    }
    CHECK(key_bits_for(1ull << 63) == 64 && key_bits_for(~0ull) == 64);
    printf(failures ? "%d checks FAILED\n" : "ws_layout_check ok\n", failures);
    return failures ? 1 : 0;
}

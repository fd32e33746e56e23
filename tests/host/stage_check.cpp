// stage_check.cpp - checks htscodecs_amd/csrc/r4x16_stage.h on the host, alone: the slot planner and the one layout every
// host-buffer call stages its batch with, over item counts around the 256-byte steps of the per-item arrays, 1 to 4
// slots per block, with and without planes, order array and gather descriptors, and both paddings in use.
// Built with -fsanitize=address,undefined and run as a program of its own (tests/test_stage_cpu.py); prints one line
// per failed check and exits 1, or "stage_check: ok" and 0.
#include "r4x16_stage.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int g_failed = 0;
#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        if (!(cond)) {                                                                \
            if (++g_failed <= 20) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                             \
    } while (0)

struct Piece { const char *name; uint8_t *p; size_t bytes; uint8_t tag; };

struct Case { size_t n, k; bool planes, order, pk; size_t pad, align; unsigned shift; };

static void describe(const Case &c, char *buf, size_t len)
{
    snprintf(buf, len, "n %zu k %zu planes %d order %d pk %d pad %zu align %zu shift %u", c.n, c.k, (int)c.planes, (int)c.order, (int)c.pk,
             c.pad, c.align, c.shift);
}

// slots: monotone, every slot of size + pad bytes at least, the last one inside the total
static void check_slots(const char *what, const char *which, const std::vector<uint32_t> &size, size_t k, size_t pad, size_t align,
                        const std::vector<uint64_t> &off, size_t total)
{
    const size_t items = size.size() * k;
    CHECK(off[0] == 0, "%s: %s slot 0 at %llu", what, which, (unsigned long long)off[0]);
    for (size_t it = 0; it < items; it++) {
        const size_t need = (size_t)size[it / k] + pad;
        const uint64_t next = it + 1 < items ? off[it + 1] : (uint64_t)total;
        CHECK(next >= off[it] && next - off[it] >= need, "%s: %s slot %zu [%llu, %llu) holds less than %zu", what, which, it,
              (unsigned long long)off[it], (unsigned long long)next, need);
        CHECK(off[it] % align == 0, "%s: %s slot %zu at %llu", what, which, it, (unsigned long long)off[it]);
    }
}

static void check_case(const Case &c)
{
    static const uint32_t sizes[] = {0, 1, 239, 240, 241, 255, 256, 4096};
    const size_t ns = sizeof(sizes) / sizeof(sizes[0]);
    char what[160];
    describe(c, what, sizeof(what));

    std::vector<uint32_t> isz(c.n), cap(c.n);
    for (size_t i = 0; i < c.n; i++) { isz[i] = sizes[(i + c.shift) % ns]; cap[i] = sizes[(i * 3 + c.shift + 1) % ns]; }
    const size_t items = c.n * c.k;
    std::vector<uint64_t> in_off(c.n), out_off(items);
    const size_t in_tot = r4x16_stage_slots(isz.data(), c.n, c.pad, c.align, in_off.data());
    const size_t out_tot = r4x16_stage_slots(cap.data(), c.n, c.pad, c.align, out_off.data(), c.k);
    check_slots(what, "input", isz, 1, c.pad, c.align, in_off, in_tot);
    check_slots(what, "output", cap, c.k, c.pad, c.align, out_off, out_tot);
    // K slots per block are a parameter, not a second plan: the same as one slot each of a batch with every block K times
    {
        std::vector<uint32_t> rep(items);
        std::vector<uint64_t> flat(items);
        for (size_t it = 0; it < items; it++) rep[it] = cap[it / c.k];
        const size_t tot = r4x16_stage_slots(rep.data(), items, c.pad, c.align, flat.data());
        CHECK(tot == out_tot && flat == out_off, "%s: k slots per block differ from the flat plan", what);
    }

    // (the arith batch asks for 16 bytes behind its unpadded slots: region sizes that are no multiples of 256)
    const size_t tail = c.pad ? 0 : 16, in_bytes = in_tot + tail, out_bytes = out_tot + tail;
    const size_t plane_bytes = c.planes ? in_bytes : 0, pk_count = c.pk ? c.n : 0;
    StageLayout D, L;
    const size_t dry = r4x16_stage_layout(&D, nullptr, items, in_bytes, plane_bytes, out_bytes, c.order, pk_count);
    CHECK(dry % 256 == 0, "%s: a total of %zu", what, dry);
    CHECK(!D.in && !D.planes && !D.out && !D.in_off && !D.out_off && !D.in_size && !D.cap && !D.osz && !D.status && !D.order && !D.pk,
          "%s: a dry run handed out a pointer", what);
    uint8_t *arena = (uint8_t *)malloc(dry ? dry : 1);          // exactly the dry run's size: a write beyond it is a finding
    const size_t real = r4x16_stage_layout(&L, arena, items, in_bytes, plane_bytes, out_bytes, c.order, pk_count);
    CHECK(real == dry, "%s: the dry run says %zu, the real run ends at %zu", what, dry, real);
    CHECK((L.planes != nullptr) == c.planes && (L.order != nullptr) == c.order && (L.pk != nullptr) == c.pk,
          "%s: an optional piece is there or not against the arguments", what);

    std::vector<Piece> pieces;
    pieces.push_back({"in", L.in, in_bytes, 0x11});
    if (L.planes) pieces.push_back({"planes", L.planes, plane_bytes, 0x22});
    pieces.push_back({"out", L.out, out_bytes, 0x33});
    pieces.push_back({"in_off", (uint8_t *)L.in_off, items * 8, 0x44});
    pieces.push_back({"out_off", (uint8_t *)L.out_off, items * 8, 0x55});
    pieces.push_back({"in_size", (uint8_t *)L.in_size, items * 4, 0x66});
    pieces.push_back({"cap", (uint8_t *)L.cap, items * 4, 0x77});
    pieces.push_back({"osz", (uint8_t *)L.osz, items * 4, 0x88});
    pieces.push_back({"status", (uint8_t *)L.status, items * 4, 0x99});
    if (L.order) pieces.push_back({"order", (uint8_t *)L.order, items * 4, 0xaa});
    if (L.pk) pieces.push_back({"pk", (uint8_t *)L.pk, pk_count * sizeof(PackDesc), 0xbb});
    CHECK(L.in == arena, "%s: the input region starts %td bytes into the arena", what, L.in - arena);
    for (size_t a = 0; a < pieces.size(); a++) {
        const Piece &A = pieces[a];
        CHECK((size_t)(A.p - arena) % 256 == 0, "%s: %s at %td", what, A.name, A.p - arena);
        CHECK(A.p >= arena && (size_t)(A.p - arena) + A.bytes <= dry, "%s: %s [%td, +%zu) leaves the arena of %zu", what, A.name, A.p - arena,
              A.bytes, dry);
        for (size_t b = a + 1; b < pieces.size(); b++) {
            const Piece &B = pieces[b];
            CHECK(A.p + A.bytes <= B.p || B.p + B.bytes <= A.p, "%s: %s [%td, +%zu) and %s [%td, +%zu) overlap", what, A.name, A.p - arena,
                  A.bytes, B.name, B.p - arena, B.bytes);
        }
    }
    if (L.order)
        CHECK((uint8_t *)L.order >= (uint8_t *)(L.status + items) || (uint8_t *)(L.order + items) <= (uint8_t *)L.status,
              "%s: the order array lies inside the status array's piece", what);
    // regions whose sizes are multiples of 256 follow each other without a gap (the gathers write from `in` into `planes`)
    if (c.align == 256) {
        CHECK((L.planes ? L.planes : L.out) == L.in + in_tot, "%s: a gap behind the input region", what);
        if (L.planes) CHECK(L.out == L.planes + plane_bytes, "%s: a gap behind the planes", what);
    }

    // the write pass: every byte of every slot, the planes, every element of every array through its own type - each
    // piece with a value of its own, and at the end no piece holds another's
    memset(arena, 0, dry);
    for (size_t i = 0; i < c.n; i++) memset(L.in + in_off[i], 0x11, (size_t)isz[i] + c.pad);
    if (L.planes) memset(L.planes, 0x22, plane_bytes);
    for (size_t it = 0; it < items; it++) memset(L.out + out_off[it], 0x33, (size_t)cap[it / c.k] + c.pad);
    for (size_t it = 0; it < items; it++) {
        L.in_off[it] = 0x4444444444444444ull; L.out_off[it] = 0x5555555555555555ull;
        L.in_size[it] = 0x66666666u; L.cap[it] = 0x77777777u; L.osz[it] = 0x88888888u;
        L.status[it] = (int32_t)0x99999999u;
        if (L.order) L.order[it] = (int32_t)0xaaaaaaaau;
    }
    for (size_t i = 0; i < pk_count; i++) { L.pk[i].src = L.pk[i].dst = 0xbbbbbbbbbbbbbbbbull; L.pk[i].len = L.pk[i].pad = 0xbbbbbbbbu; }
    for (const Piece &P : pieces) {
        const bool slots = P.p == L.in || P.p == L.out;          // (between two slots lies what the alignment left: zeros)
        size_t wrong = 0;
        for (size_t b = 0; b < P.bytes; b++) wrong += P.p[b] != P.tag && !(slots && P.p[b] == 0);
        CHECK(wrong == 0, "%s: %zu bytes of %s hold something else than what was written there", what, wrong, P.name);
    }
    free(arena);
}

int main()
{
    const size_t counts[] = {1, 31, 32, 33, 64, 65, 1000};
    size_t cases = 0;
    for (size_t n : counts)
        for (size_t k = 1; k <= 4; k++)
            for (int flags = 0; flags < 8; flags++)
                for (int padding = 0; padding < 2; padding++)
                    for (unsigned shift = 0; shift < 8; shift++) {              // every size at every position of the cycle
                        Case c;
                        c.n = n; c.k = k; c.planes = flags & 1; c.order = flags & 2; c.pk = flags & 4;
                        c.pad = padding ? 0 : 16; c.align = padding ? 16 : 256;    // the rANS calls; the arith batch
                        c.shift = shift;
                        check_case(c);
                        cases++;
                    }
    if (g_failed) { printf("stage_check: %d checks failed in %zu cases\n", g_failed, cases); return 1; }
    printf("stage_check: ok\n");
    return 0;
}

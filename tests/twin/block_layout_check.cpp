// Prints what csrc/pmv_block.h and csrc/backend_layout.h compute, one record per line as "kind key=value ...", for
// tests/test_block_layout.py to compare with the formulas written out there. Host-only: it includes nothing but the two headers.
#include "pmv_block.h"
#include "backend_layout.h"
#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace pmv;

#define F(x) printf(" " #x "=%zu", (size_t)L.x)

static void pnp(size_t m, size_t it) {
    const PnPLayout L = pnp_layout(m, it);
    printf("pnp m=%zu it=%zu", m, it); F(K); F(obj); F(img); F(samples); F(in_bytes); F(out); F(info); F(done); F(inliers); F(total); printf("\n");
}
static void ba(size_t nc, size_t np, size_t no) {
    const BaIoLayout L = ba_io_layout(nc, np, no);
    printf("ba nc=%zu np=%zu no=%zu", nc, np, no); F(summary); F(cams); F(pts); F(obs); F(K); F(cam_idx); F(pt_idx); F(pstart); F(plist); F(cstart); F(clist); F(erec);
    F(io_bytes); F(done); F(out_bytes); F(total); printf("\n");
}
static void dlt(size_t n) {
    const DltLayout L = dlt_layout(n);
    printf("dlt n=%zu", n); F(P); F(q1); F(q2); F(mask_in); F(in_bytes); F(out); F(Q); F(mask); F(total); printf("\n");
}
static void fivepoint(size_t n, size_t h) {
    const FivePointLayout L = fivepoint_layout(n, h);
    printf("fivepoint n=%zu h=%zu", n, h); F(q1); F(q2); F(samples); F(in_bytes); F(out); F(models); F(n_models); F(counts); F(total); printf("\n");
}
static void whole(const char* kind, const WholeLayout& L, size_t n) {
    printf("%s n=%zu", kind, n); F(rec); F(p1); F(p2); F(iters); F(in_bytes); F(out); F(info); F(done); F(mask); F(total); printf("\n");
}

// every n up to the context's max_tracks: what each call needs of each block it is carved from
static void fits(int mt, int nc, int np, int no) {
    const BackendCaps L = backend_caps(mt, nc, np, no);
    printf("caps mt=%d nc=%d np=%d no=%d", mt, nc, np, no); F(ba_io); F(pnp_in); F(pnp_out); F(tri_in); F(tri_out); F(ess_in); F(fund_in); F(h_stage); printf("\n");
    for (size_t n = 0; n <= (size_t)mt; n++) {
        for (size_t it : {(size_t)1, (size_t)MAX_HYP}) { const PnPLayout P = pnp_layout(n, it); printf("fit mt=%d kind=pnp n=%zu k=%zu in=%zu out=%zu total=%zu\n", mt, n, it, P.in_bytes, P.total - P.out, P.total); }
        for (size_t h : {(size_t)1, (size_t)FP_MAX_HYP}) { const FivePointLayout P = fivepoint_layout(n, h); printf("fit mt=%d kind=fivepoint n=%zu k=%zu in=%zu out=%zu total=%zu\n", mt, n, h, P.in_bytes, P.total - P.out, P.total); }
        const DltLayout D = dlt_layout(n);
        printf("fit mt=%d kind=dlt n=%zu k=0 in=%zu out=%zu total=%zu\n", mt, n, D.in_bytes, D.total - D.out, D.total);
        const WholeLayout E = essential_layout(n), Fu = fundamental_layout(n);
        printf("fit mt=%d kind=essential n=%zu k=0 in=%zu out=%zu total=%zu\n", mt, n, E.in_bytes, E.total - E.out, E.total);
        printf("fit mt=%d kind=fundamental n=%zu k=0 in=%zu out=%zu total=%zu\n", mt, n, Fu.in_bytes, Fu.total - Fu.out, Fu.total);
    }
    const BaIoLayout B = ba_io_layout((size_t)nc, (size_t)np, (size_t)no);   // (the io block grows with each of the three: its largest is at the maxima)
    printf("fit mt=%d kind=ba n=0 k=0 in=%zu out=%zu total=%zu\n", mt, B.io_bytes, B.out_bytes, B.total);
}

// one scripted sequence of takes, the last two past the capacity; every span handed out is written (the sanitizer build watches the stores)
template <class T> static void take(Carve& c, const char* run, int i, size_t count, size_t align) {
    const Carved<T> t = align ? c.take<T>(count, align) : c.take<T>(count);
    if (t.h) memset(t.h, 0x5a, count * sizeof(T));
    if (t.d) memset(t.d, 0xa5, count * sizeof(T));
    printf("carve run=%s i=%d size=%zu align=%zu off=%zu h=%td d=%td bytes=%zu overflow=%d\n", run, i, count * sizeof(T), align ? align : alignof(T), t.off,
           t.h ? (char*)t.h - c.hb : (ptrdiff_t)-1, t.d ? (char*)t.d - c.db : (ptrdiff_t)-1, c.bytes(), (int)c.overflow);
}
static void script(Carve c, const char* run) {
    take<char>(c, run, 0, 3, 0); take<double>(c, run, 1, 2, 0); take<int>(c, run, 2, 5, 0); take<char>(c, run, 3, 1, 0); take<float>(c, run, 4, 7, 16);
    take<uint8_t>(c, run, 5, 0, 0); take<double>(c, run, 6, 1, 64); take<short>(c, run, 7, 9, 0);
    c.skip_to(32);
    printf("carve run=%s i=8 size=0 align=32 off=%zu h=-1 d=-1 bytes=%zu overflow=%d\n", run, c.bytes(), c.bytes(), (int)c.overflow);
    take<double>(c, run, 9, 11, 0);    // ends exactly at the capacity of the real run
    take<char>(c, run, 10, 1, 0);      // one byte too many
    take<double>(c, run, 11, 4, 0);    // and further
}

int main() {
    printf("const MAX_HYP=%d FP_MAX_HYP=%d PNP_HDR=%zu ESS_HDR=%zu ESS_OUT_HDR=%zu PNP_OUT_INFO=%zu PNP_OUT_DONE=%zu PNP_OUT_INLIERS=%zu ESS_OUT_INFO=%zu ESS_OUT_DONE=%zu BA_SUM_SLOTS=%d BA_SUM_DONE=%d\n",
           MAX_HYP, FP_MAX_HYP, PNP_HDR, ESS_HDR, ESS_OUT_HDR, PNP_OUT_INFO, PNP_OUT_DONE, PNP_OUT_INLIERS, ESS_OUT_INFO, ESS_OUT_DONE, BA_SUM_SLOTS, BA_SUM_DONE);
    for (size_t n : {0, 1, 5, 15, 63, 64, 2000}) {
        for (size_t it : {(size_t)1, (size_t)MAX_HYP}) pnp(n, it);
        for (size_t h : {(size_t)1, (size_t)FP_MAX_HYP}) fivepoint(n, h);
        dlt(n);
        whole("essential", essential_layout(n), n);
        whole("fundamental", fundamental_layout(n), n);
        for (size_t nc : {1, 4, 32}) for (size_t np : {1, 5, 63}) ba(nc, np, n);   // (n observations)
    }
    ba(4, 32, 96); ba(32, 8192, 65536);
    fits(64, 4, 32, 96);             // a small context
    fits(4096, 32, 8192, 65536);     // the benchmark's
    alignas(64) static char host[248 + 64], dev[248 + 64];   // 248 = where take 9 of the script ends; the 64 behind it must stay untouched
    memset(host, 0, sizeof(host)); memset(dev, 0, sizeof(dev));
    script(Carve(), "dry");
    script(Carve(host, dev, 248), "real");
    for (int i = 248; i < 248 + 64; i++) if (host[i] || dev[i]) { printf("carve-wrote-past-capacity at=%d\n", i); return 1; }
    return 0;
}

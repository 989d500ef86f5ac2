// jni_measures_test.cc -- TEST INFRASTRUCTURE: drives the measures natives of the JNI shim
// (cov-tiles_amd/jni/covt_jni.cc: GpuCovtBatch.measuresBytes / measuresColumns / geometryMeasures) the way a JVM would,
// through a hand-built JNIEnv function table (tests/jni/jni.h), without a JDK.
//
// Reads cases from stdin, one per line:   <mode> S1 S2 ... | <hex of the tiles back to back>
// (tiles of sizes S1, S2, ... packed at 16-byte aligned offsets of one direct buffer) and prints
//   ok <measures bytes> <hex of the measuresColumns long[]> <hex of the geometryMeasures long[]> <hex of the output buffer>
//   or: exc <exception class>
// Modes: measures (a direct output buffer of measuresBytes()), short (one byte less), heap (not a direct buffer:
// GetDirectBufferAddress returns NULL, as a JVM's does for a heap ByteBuffer).
#include <jni.h>

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#define BFN(name) Java_com_covt_decoder_gpu_GpuCovtBatch_##name
extern "C" {
jlong BFN(create)(JNIEnv*, jclass, jobject, jlongArray, jlongArray, jint, jint, jint);
void BFN(destroy)(JNIEnv*, jclass, jlong);
jlong BFN(measuresBytes)(JNIEnv*, jclass, jlong);
jlongArray BFN(measuresColumns)(JNIEnv*, jclass, jlong);
jlongArray BFN(geometryMeasures)(JNIEnv*, jclass, jlong, jobject, jobject);
}

namespace {

struct Obj {
    enum Kind { CLASS, ARRAY, DIRECT } kind;
    std::string cls;
    int elem = 1;
    std::vector<uint8_t> data;
};
std::vector<Obj*> g_heap;
std::string g_exc;

Obj* make(Obj::Kind k) {
    g_heap.push_back(new Obj{k});
    return g_heap.back();
}
template <class T> Obj* O(T p) { return reinterpret_cast<Obj*>(p); }
template <class T> T J(Obj* o) { return reinterpret_cast<T>(o); }

jclass FindClass(JNIEnv*, const char* name) {
    Obj* c = make(Obj::CLASS);
    c->cls = name;
    return J<jclass>(c);
}
jint ThrowNew(JNIEnv*, jclass c, const char*) {
    if (g_exc.empty()) g_exc = O(c)->cls;
    return 0;
}
jsize GetArrayLength(JNIEnv*, jarray a) { return (jsize)(O(a)->data.size() / (size_t)O(a)->elem); }
Obj* new_array(jsize n, int elem) {
    Obj* a = make(Obj::ARRAY);
    a->elem = elem;
    a->data.assign((size_t)n * (size_t)elem, 0);
    return a;
}
jlongArray NewLongArray(JNIEnv*, jsize n) { return J<jlongArray>(new_array(n, 8)); }
void region(Obj* a, jsize s, jsize n, void* dst, const void* src) {
    const size_t e = (size_t)a->elem;
    if (s < 0 || n < 0 || (size_t)(s + n) * e > a->data.size()) {
        g_exc = "java/lang/ArrayIndexOutOfBoundsException";
        return;
    }
    if (dst) std::memcpy(dst, a->data.data() + s * e, n * e);
    else std::memcpy(a->data.data() + s * e, src, n * e);
}
void GetLongArrayRegion(JNIEnv*, jlongArray a, jsize s, jsize n, jlong* b) { region(O(a), s, n, b, nullptr); }
void SetLongArrayRegion(JNIEnv*, jlongArray a, jsize s, jsize n, const jlong* b) { region(O(a), s, n, nullptr, b); }
void* GetDirectBufferAddress(JNIEnv*, jobject b) { return O(b)->kind == Obj::DIRECT ? O(b)->data.data() : nullptr; }
jlong GetDirectBufferCapacity(JNIEnv*, jobject b) { return O(b)->kind == Obj::DIRECT ? (jlong)O(b)->data.size() : -1; }

JNINativeInterface_ make_table() {
    JNINativeInterface_ t{};
    t.slot[JNI_SLOT_FindClass] = (void*)&FindClass;
    t.slot[JNI_SLOT_ThrowNew] = (void*)&ThrowNew;
    t.slot[JNI_SLOT_GetArrayLength] = (void*)&GetArrayLength;
    t.slot[JNI_SLOT_NewLongArray] = (void*)&NewLongArray;
    t.slot[JNI_SLOT_GetLongArrayRegion] = (void*)&GetLongArrayRegion;
    t.slot[JNI_SLOT_SetLongArrayRegion] = (void*)&SetLongArrayRegion;
    t.slot[JNI_SLOT_GetDirectBufferAddress] = (void*)&GetDirectBufferAddress;
    t.slot[JNI_SLOT_GetDirectBufferCapacity] = (void*)&GetDirectBufferCapacity;
    return t;
}

std::vector<uint8_t> unhex(const std::string& h) {
    std::vector<uint8_t> v;
    v.reserve(h.size() / 2);
    auto nib = [](char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; };
    for (size_t i = 0; i + 1 < h.size(); i += 2) v.push_back((uint8_t)(nib(h[i]) * 16 + nib(h[i + 1])));
    return v;
}
std::string hex(const std::vector<uint8_t>& v) {
    static const char* d = "0123456789abcdef";
    std::string s;
    s.reserve(2 * v.size());
    for (uint8_t b : v) {
        s += d[b >> 4];
        s += d[b & 15];
    }
    return s;
}

}  // namespace

int main() {
    JNINativeInterface_ table = make_table();
    JNIEnv_ env_s{&table};
    JNIEnv* env = &env_s;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        const size_t bar = line.find('|');
        std::istringstream is(line.substr(0, bar));
        std::string m;
        is >> m;
        std::vector<long long> a;
        long long x;
        while (is >> x) a.push_back(x);
        std::string hx = bar == std::string::npos ? "" : line.substr(bar + 1);
        hx.erase(0, hx.find_first_not_of(' '));
        const std::vector<uint8_t> in = unhex(hx);
        if (m != "measures" && m != "short" && m != "heap") {
            std::cerr << "unknown mode " << m << "\n";
            return 2;
        }
        g_exc.clear();
        Obj* tiles = make(Obj::DIRECT);
        const size_t nt = a.size();
        Obj* offs = new_array((jsize)nt, 8);
        Obj* sizes = new_array((jsize)nt, 8);
        size_t src = 0;
        for (size_t k = 0; k < nt; ++k) {
            tiles->data.resize((tiles->data.size() + 15) & ~(size_t)15, 0);
            const int64_t o = (int64_t)tiles->data.size(), sz = (int64_t)a[k];
            if (src + (size_t)a[k] > in.size()) {
                std::cerr << "tile sizes exceed the input\n";
                return 2;
            }
            std::memcpy(offs->data.data() + 8 * k, &o, 8);
            std::memcpy(sizes->data.data() + 8 * k, &sz, 8);
            tiles->data.insert(tiles->data.end(), in.begin() + (std::ptrdiff_t)src,
                               in.begin() + (std::ptrdiff_t)(src + (size_t)a[k]));
            src += (size_t)a[k];
        }
        tiles->data.resize(tiles->data.size() + 4096, 0);  // COVT_INPUT_PADDING
        const jlong h = BFN(create)(env, nullptr, J<jobject>(tiles), J<jlongArray>(offs), J<jlongArray>(sizes), 0, 0, 0);
        if (!g_exc.empty()) {
            std::cout << "exc " << g_exc << "\n";
            continue;
        }
        const jlong nb = BFN(measuresBytes)(env, nullptr, h);
        jlongArray cols = BFN(measuresColumns)(env, nullptr, h);
        Obj* out = make(m == "heap" ? Obj::ARRAY : Obj::DIRECT);
        out->data.assign((size_t)(m == "short" ? nb - 1 : nb), 0x5A);
        jlongArray res = g_exc.empty() ? BFN(geometryMeasures)(env, nullptr, h, J<jobject>(tiles), J<jobject>(out)) : nullptr;
        BFN(destroy)(env, nullptr, h);
        if (!g_exc.empty()) {
            std::cout << (res ? "bad returned-with-exception" : "exc " + g_exc) << "\n";
        } else if (!res || !cols) {
            std::cout << "bad null-without-exception\n";
        } else {
            std::cout << "ok " << nb << " " << hex(O(cols)->data) << " " << hex(O(res)->data) << " " << hex(out->data)
                      << "\n";
        }
    }
    std::cout.flush();
    for (Obj* o : g_heap) delete o;
    return 0;
}

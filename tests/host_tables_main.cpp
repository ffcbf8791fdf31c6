// Stand-alone check of avec_amd/csrc/host_tables.h (no HIP): the rules of the reduction-workspace registry and of the LDS opt-in table, then both classes
// hammered from two threads.  tests/test_host_tables.py builds this with -fsanitize=thread and runs it; exit status 0 and "host_tables OK" mean every rule held.
#include "host_tables.h"
#include <stdio.h>
#include <stdlib.h>
#include <thread>

#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static char g_buf[8][16];                       // addresses only: nothing is read or written through them
static void* buf(int i) { return g_buf[i]; }
static const void* key(int i) { return g_buf[i] + 8; }

static void registry_rules() {
  WsRegistry r;
  const size_t KB = 1024;
  REQUIRE(r.find(0, nullptr, 1) == nullptr);                                    // nothing registered
  REQUIRE(r.set_default(0, buf(0), 64 * KB));
  REQUIRE(r.find(0, key(1), 64 * KB) == buf(0) && r.find(0, key(1), 64 * KB + 1) == nullptr);      // any stream gets the default when it is large enough
  REQUIRE(r.find(1, key(1), 1) == nullptr);                                     // ... of its own device
  REQUIRE(!r.set_default(-1, buf(0), 64 * KB) && !r.set_default(WsRegistry::MAX_DEV, buf(0), 64 * KB) && r.find(WsRegistry::MAX_DEV, nullptr, 1) == nullptr);
  // a stream-bound entry beats the default, and one that is too small gives none (not the larger default)
  REQUIRE(r.set_stream(0, key(1), buf(1), 16 * KB));
  REQUIRE(r.find(0, key(1), 16 * KB) == buf(1) && r.find(0, key(1), 16 * KB + 1) == nullptr && r.find(0, key(2), 64 * KB) == buf(0));
  REQUIRE(r.find(1, key(1), 1) == nullptr);                                     // bound on device 0 only
  // replace in place: the same (device, stream) again takes no new entry
  REQUIRE(r.set_stream(0, key(1), buf(2), 32 * KB) && r.find(0, key(1), 32 * KB) == buf(2));
  REQUIRE(r.set_stream(0, key(2), buf(3), KB) && r.set_stream(1, key(1), buf(4), KB) && r.set_stream(1, key(3), buf(5), KB));
  REQUIRE(!r.set_stream(0, key(4), buf(6), KB));                                // the fifth stream-bound entry is refused
  REQUIRE(r.set_stream(1, key(3), buf(6), 2 * KB) && r.find(1, key(3), 2 * KB) == buf(6));          // ... a replacement still goes through
  REQUIRE(r.find(0, key(4), 64 * KB) == buf(0));
  // unregister the default with (NULL, 0): stream-bound entries stay
  REQUIRE(r.set_default(0, nullptr, 0) && r.find(0, key(4), 1) == nullptr && r.find(0, key(4), 0) == nullptr && r.find(0, key(1), 32 * KB) == buf(2));
}

static int g_calls = 0;
static size_t g_limit = 0;                      // the fake device grants up to this many bytes
static int fake_set(const void*, size_t bytes) { ++g_calls; return bytes <= g_limit ? 0 : 1000 + (int)(bytes / 1024); }

static void optin_rules() {
  LdsOptin t;
  const size_t KB = 1024;
  g_calls = 0; g_limit = 128 * KB;
  REQUIRE(t.request(0, key(0), 0, fake_set) == 0 && t.request(0, key(0), 48 * KB, fake_set) == 0 && g_calls == 0);      // at most 48 KB: no call
  REQUIRE(t.request(0, key(0), 160 * KB + 1, fake_set) == LdsOptin::TOO_LARGE && g_calls == 0);
  REQUIRE(t.request(0, key(0), 48 * KB + 1, fake_set) == 0 && g_calls == 1);
  REQUIRE(t.request(0, key(0), 48 * KB + 1, fake_set) == 0 && t.request(0, key(0), 10 * KB, fake_set) == 0 && g_calls == 1);   // same or smaller: no call
  REQUIRE(t.request(0, key(0), 80 * KB, fake_set) == 0 && g_calls == 2);                                                 // growth: one more call
  REQUIRE(t.request(0, key(0), 64 * KB, fake_set) == 0 && t.request(0, key(0), 80 * KB, fake_set) == 0 && g_calls == 2);
  REQUIRE(t.request(0, key(1), 64 * KB, fake_set) == 0 && g_calls == 3);                                                 // another kernel: its own entry
  // a refusal is remembered with its code; what was granted before still stands
  REQUIRE(t.request(0, key(0), 150 * KB, fake_set) == 1150 && g_calls == 4);
  REQUIRE(t.request(0, key(0), 150 * KB, fake_set) == 1150 && t.request(0, key(0), 160 * KB, fake_set) == 1150 && g_calls == 4);
  REQUIRE(t.request(0, key(0), 80 * KB, fake_set) == 0 && g_calls == 4);
  REQUIRE(t.request(0, key(0), 100 * KB, fake_set) == 0 && g_calls == 5);                                                // between the grant and the refusal: asked
  // two devices are independent
  REQUIRE(t.request(1, key(0), 80 * KB, fake_set) == 0 && g_calls == 6);
  REQUIRE(t.request(1, key(0), 150 * KB, fake_set) == 1150 && g_calls == 7 && t.request(1, key(0), 150 * KB, fake_set) == 1150 && g_calls == 7);
  REQUIRE(t.request(2, key(0), 150 * KB, fake_set) == 1150 && g_calls == 8);
}

static void hammer() {
  WsRegistry r; LdsOptin t;
  int calls = 0;                                 // written under the table's mutex only: the thread sanitizer reports it if request() runs `set` unlocked
  auto set = [&calls](const void*, size_t bytes) { ++calls; return bytes > 128 * 1024 ? 7 : 0; };
  auto work = [&](int me) {
    for (int i = 0; i < 20000; ++i) {
      const int dev = i & 1, k = i % 5;
      r.set_default(dev, buf(me), (size_t)(1 + (i & 7)) << 16);
      r.set_stream(dev, key(k & 1), buf(2 + me), (size_t)(1 + (i & 3)) << 16);
      void* a = r.find(dev, key(k & 1), 1 << 16); REQUIRE(a == buf(2) || a == buf(3));
      void* b = r.find(dev, key(7), 1 << 16); REQUIRE(b == buf(0) || b == buf(1));
      const size_t bytes = (size_t)(40 + (i * 7) % 120) * 1024;
      const int e = t.request(dev, key(k), bytes, set);
      REQUIRE(e == (bytes > 128 * 1024 ? 7 : 0));
    }
  };
  std::thread a(work, 0), b(work, 1);
  a.join(); b.join();
  // 2 devices x 5 kernels: sizes only grow between 48 KB and 128 KB in 1 KB steps, refusals only shrink down to 129 KB
  REQUIRE(calls >= 10 && calls <= 10 * (80 + 32));
}

int main() {
  registry_rules();
  optin_rules();
  hammer();
  puts("host_tables OK");
  return 0;
}

// Tests for key watches (cpilot/kv.hpp): the base64 decoder, the /v1/kv
// body parser, the change rule, the data model handed to templates, the
// `watches[].key` / `keyPrefix` config rules and the request path. No
// daemon, no network.
// Run via `bin/cpilot_kvtests`; exits non-zero if any check failed.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "cpilot/discovery.hpp"
#include "cpilot/json.hpp"
#include "cpilot/kv.hpp"
#include "cpilot/tmpl.hpp"
#include "cpilot/watches.hpp"

using namespace cpilot;

static int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      failures++;                                                         \
    }                                                                     \
  } while (0)
#define CHECK_EQ(a, b)                                                    \
  do {                                                                    \
    auto va = (a);                                                        \
    auto vb = (b);                                                        \
    if (!(va == vb)) {                                                    \
      fprintf(stderr, "FAIL %s:%d: %s != %s\n  got:  %s\n  want: %s\n",   \
              __FILE__, __LINE__, #a, #b, std::string(va).c_str(),        \
              std::string(vb).c_str());                                   \
      failures++;                                                         \
    }                                                                     \
  } while (0)

namespace {

// ---------- base64 ----------

void testBase64Valid() {
  // every length from 0 to 6 bytes of 00 ff 41 62 63 80
  const std::string bytes("\x00\xff" "Abc" "\x80", 6);
  const char* encoded[] = {"",         "AA==",     "AP8=",    "AP9B",
                           "AP9BYg==", "AP9BYmM=", "AP9BYmOA"};
  for (size_t n = 0; n <= 6; n++) {
    std::string out = "stale";
    CHECK(base64Decode(encoded[n], &out));
    CHECK(out == bytes.substr(0, n));
  }

  // every byte value
  const std::string all =
      "AAECAwQFBgcICQoLDA0ODxAREhMUFRYXGBkaGxwdHh8gISIjJCUmJygpKissLS4v"
      "MDEyMzQ1Njc4OTo7PD0+P0BBQkNERUZHSElKS0xNTk9QUVJTVFVWV1hZWltcXV5f"
      "YGFiY2RlZmdoaWprbG1ub3BxcnN0dXZ3eHl6e3x9fn+AgYKDhIWGh4iJiouMjY6P"
      "kJGSk5SVlpeYmZqbnJ2en6ChoqOkpaanqKmqq6ytrq+wsbKztLW2t7i5uru8vb6/"
      "wMHCw8TFxsfIycrLzM3Oz9DR0tPU1dbX2Nna29zd3t/g4eLj5OXm5+jp6uvs7e7v"
      "8PHy8/T19vf4+fr7/P3+/w==";
  std::string out;
  CHECK(base64Decode(all, &out));
  CHECK(out.size() == 256);
  for (size_t i = 0; i < out.size() && i < 256; i++)
    CHECK((unsigned char)out[i] == i);
}

void testBase64Refused() {
  const char* refused[] = {"Q",        "QQ",      "QQ=",    "QQ=Q", "=QQQ",
                           "QQ==QQ==", "QUJD\n",  "QU JD",  "QUJ-", "QUJ_"};
  for (const char* in : refused) {
    std::string out = "stale";
    if (base64Decode(in, &out)) {
      fprintf(stderr, "FAIL: base64Decode accepted \"%s\"\n", in);
      failures++;
    }
    CHECK(out.empty());
  }
  // more of the same rules
  std::string out;
  CHECK(!base64Decode("====", &out));
  CHECK(!base64Decode("Q===", &out));
  CHECK(!base64Decode("QUJD====", &out));
  CHECK(!base64Decode(std::string("QUJ\0", 4), &out));
  CHECK(!base64Decode("QUJD\r\n", &out));
  // non-zero trailing bits are accepted
  CHECK(base64Decode("QR==", &out));
  CHECK_EQ(out, std::string("A"));
  CHECK(base64Decode("QUJ=", &out));
  CHECK_EQ(out, std::string("AB"));
}

// ---------- body parser ----------

void testBodyParser() {
  std::vector<KVEntry> got;

  // Value null and Value absent are the empty value; unknown fields are
  // ignored; entries come back sorted whatever order they arrive in
  CHECK(parseKVEntries(
      R"([{"LockIndex": 0, "Key": "app/z", "Flags": 7, "Value": "emVk",
           "CreateIndex": 10, "ModifyIndex": 12, "Session": "abc"},
          {"Key": "app/null", "Flags": 0, "Value": null},
          {"Key": "app/absent"},
          {"Key": "app/a", "Flags": 1, "Value": "AP8="}])",
      &got));
  CHECK(got.size() == 4);
  if (got.size() == 4) {
    CHECK_EQ(got[0].key, std::string("app/a"));
    CHECK(got[0].value == std::string("\x00\xff", 2));
    CHECK(got[0].flags == 1);
    CHECK_EQ(got[1].key, std::string("app/absent"));
    CHECK(got[1].value.empty() && got[1].flags == 0);
    CHECK_EQ(got[2].key, std::string("app/null"));
    CHECK(got[2].value.empty());
    CHECK_EQ(got[3].key, std::string("app/z"));
    CHECK_EQ(got[3].value, std::string("zed"));
    CHECK(got[3].flags == 7);
  }
  CHECK(parseKVEntries("[]", &got));
  CHECK(got.empty());

  // not an array
  CHECK(!parseKVEntries(R"({"Key": "a", "Value": null})", &got));
  CHECK(!parseKVEntries("null", &got));
  CHECK(!parseKVEntries("", &got));
  CHECK(!parseKVEntries("[{\"Key\": \"a\"}", &got));
  // an entry without a string Key, or that is no object
  CHECK(!parseKVEntries(R"([{"Value": "QQ=="}])", &got));
  CHECK(!parseKVEntries(R"([{"Key": 7, "Value": "QQ=="}])", &got));
  CHECK(!parseKVEntries(R"([{"Key": null}])", &got));
  CHECK(!parseKVEntries(R"(["a"])", &got));
  // a bad Value in the second of two entries fails the whole body
  got.push_back(KVEntry{"stale", "", 0});
  CHECK(!parseKVEntries(
      R"([{"Key": "a", "Value": "QQ=="}, {"Key": "b", "Value": "QQ="}])",
      &got));
  CHECK(got.empty());
  // a Value or Flags of another type
  CHECK(!parseKVEntries(R"([{"Key": "a", "Value": 7}])", &got));
  CHECK(!parseKVEntries(R"([{"Key": "a", "Flags": "1"}])", &got));
}

// ---------- change rule ----------

std::vector<KVEntry> parsed(const std::string& body) {
  std::vector<KVEntry> out;
  CHECK(parseKVEntries(body, &out));
  return out;
}

void testChangeRule() {
  const auto base = parsed(
      R"([{"Key": "p/a", "Flags": 0, "Value": "QQ==", "ModifyIndex": 5},
          {"Key": "p/b", "Flags": 2, "Value": null, "ModifyIndex": 6}])");
  // same bytes, another ModifyIndex, another order: no change
  CHECK(!kvEntriesDiffer(base, base));
  CHECK(!kvEntriesDiffer(
      base,
      parsed(R"([{"Key": "p/b", "Flags": 2, "ModifyIndex": 9},
                 {"Key": "p/a", "Flags": 0, "Value": "QQ==",
                  "ModifyIndex": 9}])")));
  // value bytes
  CHECK(kvEntriesDiffer(
      base, parsed(R"([{"Key": "p/a", "Flags": 0, "Value": "Qg=="},
                       {"Key": "p/b", "Flags": 2, "Value": null}])")));
  // flags only
  CHECK(kvEntriesDiffer(
      base, parsed(R"([{"Key": "p/a", "Flags": 1, "Value": "QQ=="},
                       {"Key": "p/b", "Flags": 2, "Value": null}])")));
  // one key added, one removed, one renamed
  CHECK(kvEntriesDiffer(
      base, parsed(R"([{"Key": "p/a", "Flags": 0, "Value": "QQ=="},
                       {"Key": "p/b", "Flags": 2, "Value": null},
                       {"Key": "p/c"}])")));
  CHECK(kvEntriesDiffer(
      base, parsed(R"([{"Key": "p/a", "Flags": 0, "Value": "QQ=="}])")));
  CHECK(kvEntriesDiffer(
      base, parsed(R"([{"Key": "p/a", "Flags": 0, "Value": "QQ=="},
                       {"Key": "p/c", "Flags": 2, "Value": null}])")));
  // nothing against nothing, nothing against an empty value
  CHECK(!kvEntriesDiffer({}, {}));
  CHECK(kvEntriesDiffer({}, parsed(R"([{"Key": "p/a"}])")));
}

// ---------- data model ----------

std::string renderKV(const std::string& tmpl, const std::string& key,
                     bool prefix, const std::vector<KVEntry>& entries) {
  return Template::parse(tmpl).render(
      buildKVRenderData("mode", key, prefix, "dc2", entries));
}

void testModel() {
  const std::string scalars =
      "{{ .Name }}|{{ .Key }}|{{ .DC }}|{{ .Prefix }}|{{ .Exists }}|"
      "{{ .Healthy }}|{{ .Value }}|{{ .Flags }}|{{ len .Keys }}";
  CHECK_EQ(renderKV(scalars, "app/mode", false, {}),
           std::string("mode|app/mode|dc2|false|false|false||0|0"));
  CHECK_EQ(renderKV(scalars, "app/mode", false,
                    parsed(R"([{"Key": "app/mode", "Flags": 42,
                                "Value": "Ymx1ZQ=="}])")),
           std::string("mode|app/mode|dc2|false|true|true|blue|42|1"));
  // a prefix: .Value and .Flags stay zero, .Keys is sorted, .Rel is cut
  const auto three = parsed(
      R"([{"Key": "app/v/c", "Value": "Mw=="},
          {"Key": "app/v/a", "Flags": 1, "Value": "MQ=="},
          {"Key": "app/v/b/x", "Value": null}])");
  CHECK_EQ(renderKV(scalars, "app/v/", true, three),
           std::string("mode|app/v/|dc2|true|true|true||0|3"));
  CHECK_EQ(renderKV("{{ range .Keys }}{{ .Key }}={{ .Rel }}={{ .Value }}="
                    "{{ .Flags }};{{ end }}",
                    "app/v/", true, three),
           std::string("app/v/a=a=1=1;app/v/b/x=b/x==0;app/v/c=c=3=0;"));
  // bytes pass through: a NUL and invalid UTF-8
  std::string raw = renderKV(
      "[{{ .Value }}]", "k", false,
      parsed(R"([{"Key": "k", "Value": "YQBi/4A="}])"));
  CHECK(raw == std::string("[a\0b\xff\x80]", 7));
}

// ---------- config rules ----------

bool decodeWatches(const std::string& watchesJson5,
                   std::vector<std::shared_ptr<WatchConfig>>* out,
                   std::string* err) {
  return newWatchConfigs(parseJson5(watchesJson5), out, err);
}

void expectRejected(const std::string& watchesJson5, const std::string& want) {
  std::vector<std::shared_ptr<WatchConfig>> out;
  std::string err;
  if (decodeWatches(watchesJson5, &out, &err)) {
    fprintf(stderr, "FAIL: accepted %s\n", watchesJson5.c_str());
    failures++;
    return;
  }
  CHECK_EQ(err, want);
}

void testConfig() {
  std::vector<std::shared_ptr<WatchConfig>> out;
  std::string err;
  CHECK(decodeWatches(
      "[{name: 'mode', key: 'myapp/config/mode', interval: 5, blocking: true,"
      "  render: {source: '/etc/app/mode.ctmpl', dest: '/etc/app/mode.conf'}},"
      " {name: 'vhosts', keyPrefix: 'myapp/vhosts/', interval: 10, dc: 'dc2'},"
      " {name: 'backend', interval: 3, tag: 'blue', key: null}]",
      &out, &err));
  CHECK_EQ(err, std::string(""));
  CHECK(out.size() == 3);
  if (out.size() == 3) {
    CHECK_EQ(out[0]->name, std::string("watch.mode"));
    CHECK_EQ(out[0]->serviceName, std::string("mode"));
    CHECK(out[0]->isKey && !out[0]->keyPrefix);
    CHECK_EQ(out[0]->key, std::string("myapp/config/mode"));
    CHECK(out[0]->blocking && out[0]->poll == 5 && out[0]->render);
    CHECK(out[1]->isKey && out[1]->keyPrefix);
    CHECK_EQ(out[1]->key, std::string("myapp/vhosts/"));
    CHECK_EQ(out[1]->dc, std::string("dc2"));
    CHECK(!out[1]->blocking && !out[1]->render);
    // a service watch, as before
    CHECK(!out[2]->isKey && out[2]->key.empty());
    CHECK_EQ(out[2]->tag, std::string("blue"));
  }
  // 512 bytes are accepted, UTF-8 and spaces too
  CHECK(decodeWatches("[{name: 'kw', interval: 1, key: '" +
                          std::string(512, 'a') + "'}]",
                      &out, &err));
  CHECK(decodeWatches("[{name: 'kw', interval: 1, key: 'caf\xc3\xa9/a b'}]",
                      &out, &err));

  expectRejected("[{name: 'kw', interval: 1, key: 'a', keyPrefix: 'a/'}]",
                 "watch[kw]: key and keyPrefix are mutually exclusive");
  expectRejected("[{name: 'kw', interval: 1, key: ''}]",
                 "watch[kw].key must be a non-empty string");
  expectRejected("[{name: 'kw', interval: 1, key: 7}]",
                 "watch[kw].key must be a non-empty string");
  expectRejected("[{name: 'kw', interval: 1, keyPrefix: ''}]",
                 "watch[kw].keyPrefix must be a non-empty string");
  expectRejected("[{name: 'kw', interval: 1, key: '" + std::string(513, 'a') +
                     "'}]",
                 "watch[kw].key must be at most 512 bytes");
  expectRejected("[{name: 'kw', interval: 1, key: '/a'}]",
                 "watch[kw].key must not start with '/'");
  expectRejected("[{name: 'kw', interval: 1, keyPrefix: '/'}]",
                 "watch[kw].keyPrefix must not start with '/'");
  expectRejected("[{name: 'kw', interval: 1, key: 'a\\tb'}]",
                 "watch[kw].key must not contain control characters");
  expectRejected("[{name: 'kw', interval: 1, key: 'a\\u0000b'}]",
                 "watch[kw].key must not contain control characters");
  expectRejected("[{name: 'kw', interval: 1, keyPrefix: 'a\\u007f'}]",
                 "watch[kw].keyPrefix must not contain control characters");
  expectRejected("[{name: 'kw', interval: 1, key: 'a', tag: 'blue'}]",
                 "watch[kw].tag does not apply to a key watch");
  // the other options keep their rules
  expectRejected("[{name: 'kw', key: 'a'}]", "watch[kw].interval must be > 0");
  expectRejected("[{name: 'kw', interval: 1, key: 'a', render: '/a'}]",
                 "watch[kw].render must be an object");
  CHECK(!decodeWatches("[{name: 'Bad', interval: 1, key: 'a'}]", &out, &err));
  // a key watch shares its name with nobody, whichever comes first
  const std::string dup =
      "watch[kw]: a key watch must not share its name with another watch";
  expectRejected(
      "[{name: 'kw', interval: 1, key: 'a'}, {name: 'kw', interval: 1}]", dup);
  expectRejected(
      "[{name: 'kw', interval: 1}, {name: 'kw', interval: 1, keyPrefix: 'a'}]",
      dup);
  expectRejected("[{name: 'kw', interval: 1, key: 'a'},"
                 " {name: 'kw', interval: 1, key: 'b'}]",
                 dup);
  // two service watches of one name stay accepted
  CHECK(decodeWatches("[{name: 'kw', interval: 1}, {name: 'kw', interval: 2}]",
                      &out, &err));
}

// ---------- request path ----------

void testRequestPath() {
  CHECK_EQ(kvRequestPath("myapp/config/mode", false, ""),
           std::string("/v1/kv/myapp/config/mode"));
  CHECK_EQ(kvRequestPath("myapp/vhosts/", true, ""),
           std::string("/v1/kv/myapp/vhosts/?recurse=true"));
  CHECK_EQ(kvRequestPath("a", false, "dc2"), std::string("/v1/kv/a?dc=dc2"));
  CHECK_EQ(kvRequestPath("a/", true, "dc 2", true, 17, 10),
           std::string("/v1/kv/a/?recurse=true&dc=dc%202&index=17&wait=10s"));
  CHECK_EQ(kvRequestPath("a", false, "", true, 0, 10),
           std::string("/v1/kv/a?index=0&wait=10s"));
  // a space, '%', '?', '#' and UTF-8 are encoded; slashes stay
  CHECK_EQ(kvRequestPath("a b/50%/what?/#1/caf\xc3\xa9", false, ""),
           std::string("/v1/kv/a%20b/50%25/what%3F/%231/caf%C3%A9"));
  CHECK_EQ(kvRequestPath("a//b/", false, ""), std::string("/v1/kv/a//b/"));
  CHECK_EQ(kvRequestPath("a+b&c=d", true, ""),
           std::string("/v1/kv/a%2Bb%26c%3Dd?recurse=true"));
}

}  // namespace

int main() {
  testBase64Valid();
  testBase64Refused();
  testBodyParser();
  testChangeRule();
  testModel();
  testConfig();
  testRequestPath();
  if (failures) {
    fprintf(stderr, "%d kv test(s) failed\n", failures);
    return 1;
  }
  printf("all kv tests passed\n");
  return 0;
}

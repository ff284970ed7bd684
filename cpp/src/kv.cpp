#include "cpilot/kv.hpp"

#include <algorithm>

namespace cpilot {

namespace {

// 0-63 for a character of the standard alphabet, -1 for anything else
int base64Digit(unsigned char c) {
  if (c >= 'A' && c <= 'Z') return c - 'A';
  if (c >= 'a' && c <= 'z') return c - 'a' + 26;
  if (c >= '0' && c <= '9') return c - '0' + 52;
  if (c == '+') return 62;
  if (c == '/') return 63;
  return -1;
}

}  // namespace

bool base64Decode(const std::string& in, std::string* out) {
  out->clear();
  const size_t n = in.size();
  if (n % 4 != 0) return false;
  if (n == 0) return true;
  // padding: "xx==" or "xxx=" in the last group only
  size_t pad = 0;
  if (in[n - 1] == '=') pad = in[n - 2] == '=' ? 2 : 1;
  const size_t digits = n - pad;
  std::string bytes;
  bytes.reserve(n / 4 * 3);
  uint32_t acc = 0;
  int bits = 0;
  for (size_t i = 0; i < digits; i++) {
    int d = base64Digit((unsigned char)in[i]);
    if (d < 0) return false;  // '=' before the padding lands here too
    acc = (acc << 6) | (uint32_t)d;
    bits += 6;
    if (bits >= 8) {
      bits -= 8;
      bytes += (char)((acc >> bits) & 0xff);
    }
  }
  // whatever is left in `acc` are the trailing bits: ignored
  *out = std::move(bytes);
  return true;
}

bool parseKVEntries(const std::string& body, std::vector<KVEntry>* out) {
  out->clear();
  std::vector<KVEntry> entries;
  try {
    Json doc = parseJson5(body);
    if (!doc.isArray()) return false;
    for (auto& e : doc.array()) {
      if (!e.isObject()) return false;
      const Json* key = e.find("Key");
      if (!key || !key->isString()) return false;
      KVEntry entry;
      entry.key = key->str();
      if (const Json* flags = e.find("Flags")) {
        if (!flags->isNumber()) return false;
        entry.flags = (uint64_t)flags->asInt();
      }
      if (const Json* value = e.find("Value")) {
        if (value->isString()) {
          if (!base64Decode(value->str(), &entry.value)) return false;
        } else if (!value->isNull()) {
          return false;
        }
      }
      entries.push_back(std::move(entry));
    }
  } catch (const std::exception&) {
    return false;
  }
  std::stable_sort(entries.begin(), entries.end(),
                   [](const KVEntry& a, const KVEntry& b) {
                     return a.key < b.key;
                   });
  *out = std::move(entries);
  return true;
}

bool kvEntriesDiffer(const std::vector<KVEntry>& a,
                     const std::vector<KVEntry>& b) {
  return !(a == b);
}

bool validateKVKey(const Json& raw, std::string* out, std::string* err) {
  if (!raw.isString() || raw.str().empty()) {
    *err = "must be a non-empty string";
    return false;
  }
  const std::string& key = raw.str();
  if (key.size() > 512) {
    *err = "must be at most 512 bytes";
    return false;
  }
  if (key[0] == '/') {
    *err = "must not start with '/'";
    return false;
  }
  for (unsigned char c : key) {
    if (c < 0x20 || c == 0x7f) {
      *err = "must not contain control characters";
      return false;
    }
  }
  *out = key;
  return true;
}

Json buildKVRenderData(const std::string& name, const std::string& key,
                       bool prefix, const std::string& dc,
                       const std::vector<KVEntry>& entries) {
  JsonArray keys;
  for (auto& e : entries) {
    std::string rel = e.key.compare(0, key.size(), key) == 0
                          ? e.key.substr(key.size())
                          : e.key;
    keys.push_back(Json(JsonObject{
        {"Key", Json(e.key)},
        {"Rel", Json(std::move(rel))},
        {"Value", Json(e.value)},
        {"Flags", Json((int64_t)e.flags)},
    }));
  }
  const bool exists = !entries.empty();
  const bool single = !prefix && exists;
  return Json(JsonObject{
      {"Name", Json(name)},
      {"Key", Json(key)},
      {"DC", Json(dc)},
      {"Prefix", Json(prefix)},
      {"Exists", Json(exists)},
      {"Healthy", Json(exists)},
      {"Value", Json(single ? entries[0].value : std::string())},
      {"Flags", Json(single ? (int64_t)entries[0].flags : (int64_t)0)},
      {"Keys", Json(std::move(keys))},
  });
}

}  // namespace cpilot

// Consul key/value entries for key watches: the base64 decoder, the
// /v1/kv response parser, the change rule, the key rules of the config and
// the data model handed to render templates. Pure functions; the queries
// themselves are ConsulBackend::kvGet and kvGetBlocking.
// The reference has no KV support: the contract is docs/30-configuration.md,
// "Watching Consul keys".
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "cpilot/json.hpp"

namespace cpilot {

// A response body larger than this is a failed query (Consul caps one
// value at 512 KiB).
constexpr size_t kKVMaxBody = 4u << 20;

struct KVEntry {
  std::string key;
  std::string value;  // decoded bytes, carried unchanged
  uint64_t flags = 0;
};

inline bool operator==(const KVEntry& a, const KVEntry& b) {
  return a.key == b.key && a.value == b.value && a.flags == b.flags;
}

// Standard alphabet, padding required. Refused: any other character (white
// space included), a length that is no multiple of 4, and '=' anywhere but
// in the last two positions. Non-zero trailing bits are accepted, as Go's
// and Python's decoders do. On failure *out is left empty.
bool base64Decode(const std::string& in, std::string* out);

// Decode a /v1/kv response body: a JSON array of objects with a string
// `Key`, a numeric `Flags` (0 when absent) and a `Value` that is base64, or
// null or absent for an empty value. Other fields are ignored. Anything
// else fails the whole body. Entries come back sorted by key, bytewise.
bool parseKVEntries(const std::string& body, std::vector<KVEntry>* out);

// The change rule: the two sets differ as (Key, Value bytes, Flags). Both
// must be sorted by key, as parseKVEntries leaves them.
bool kvEntriesDiffer(const std::vector<KVEntry>& a,
                     const std::vector<KVEntry>& b);

// The rules of watches[].key and watches[].keyPrefix: a non-empty string of
// at most 512 bytes without a leading '/', a byte below 0x20 or 0x7f. On
// failure sets err to "must ..." (the caller names the field).
bool validateKVKey(const Json& raw, std::string* out, std::string* err);

// What a key watch's render template sees as ".": Name, Key, DC, Prefix,
// Exists (also as Healthy), Value and Flags of a single key ("" and 0 when
// missing or for a prefix), and Keys sorted by key, each with Key, Rel (Key
// without the configured key or prefix), Value and Flags.
Json buildKVRenderData(const std::string& name, const std::string& key,
                       bool prefix, const std::string& dc,
                       const std::vector<KVEntry>& entries);

}  // namespace cpilot

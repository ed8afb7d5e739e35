#!/usr/bin/env python3
"""Render etc/config.json from a template + metadata JSON.

The reference's config is rendered by the SAPI config-agent from a
mustache template (sapi_manifests/binder/template). This is the
standalone equivalent: {{KEY}} substitution from a metadata file, plus
optional blocks: the lines between a `{{#KEY}}` line and a `{{/KEY}}`
line are kept when KEY is set and dropped, markers included, when not.

ZK_SERVERS (metadata key, else the environment variable of that name)
names the ZooKeeper servers, as a connect string `host[:port],host[:port]`
or as a list of {"host", "port"}; it renders as zookeeper.servers, the
array the reference's registrar template carries. ZK_PORT (default 2181)
is the port of entries without one. Without ZK_SERVERS the block is
dropped and binderd falls back to ZK_HOST / zookeeper.host.

usage: render-config.py template.json.in metadata.json > config.json
"""
import json
import os
import re
import sys

template = open(sys.argv[1]).read()
meta = json.load(open(sys.argv[2]))


def zk_servers(value, default_port):
    """A connect string as [{"host", "port"}]; binderd does the strict
    parsing (native/zk/hostlist.hpp) and refuses what is malformed."""
    if not isinstance(value, str):
        return value
    out = []
    for entry in value.split(","):
        host, colon, port = entry.strip().partition(":")
        if not host or "/" in entry or "[" in entry or \
                (colon and not port.isdigit()):
            sys.exit(f"render-config: bad ZK_SERVERS entry {entry!r}")
        out.append({"host": host,
                    "port": int(port) if colon else default_port})
    return out


servers = meta.get("ZK_SERVERS") or os.environ.get("ZK_SERVERS")
if servers:
    meta["ZK_SERVERS"] = zk_servers(
        servers, int(meta.get("ZK_PORT") or os.environ.get("ZK_PORT")
                     or 2181))
else:
    meta.pop("ZK_SERVERS", None)


def block(m):
    return m.group(2) if meta.get(m.group(1)) else ""


def sub(m):
    key = m.group(1).strip()
    v = meta.get(key, "")
    return json.dumps(v)[1:-1] if isinstance(v, str) else json.dumps(v)


out = re.sub(r"^\{\{#(\w+)\}\}\n(.*?)^\{\{/\1\}\}\n", block, template,
             flags=re.M | re.S)
out = re.sub(r"\{\{([^}]+)\}\}", sub, out)
json.loads(out)  # validate
sys.stdout.write(out)

// k8_shim.js -- runs an unmodified pangene.js under node, standing in for the k8 runtime it was written for.
//   node k8_shim.js /path/to/pangene.js <command> [arguments...]
// It provides what the script uses of k8: print() (arguments joined by TAB, one line on stdout), File (plain or gzipped,
// readline into a Bytes buffer; a trailing CR is dropped as k8's line reader does), Bytes, exit() and `arguments`.  Node 12
// does not parse private class members, so `#name(` and `this.#name` are renamed to plain members when the script is loaded.
"use strict";
const fs = require("fs");
const zlib = require("zlib");
const vm = require("vm");

let out = [];
function flush() { if (out.length) { fs.writeSync(1, out.join("")); out = []; } }
global.print = function (...a) { out.push(a.join("\t") + "\n"); if (out.length >= 4096) flush(); };
global.exit = function (code) { flush(); process.exit(code); };

global.Bytes = class Bytes {
	constructor() { this.s = ""; }
	toString() { return this.s; }
	destroy() {}
};
global.File = class File {
	constructor(fn) {
		let buf = fs.readFileSync(fn == null || fn == "-" ? 0 : fn);
		if (buf.length >= 2 && buf[0] == 0x1f && buf[1] == 0x8b) buf = zlib.gunzipSync(buf);
		const text = buf.toString("latin1");
		this.lines = text.split("\n");
		if (this.lines.length && this.lines[this.lines.length - 1] == "") this.lines.pop();
		this.i = 0;
	}
	readline(b) {
		if (this.i >= this.lines.length) return -1;
		let l = this.lines[this.i++];
		if (l.length > 0 && l[l.length - 1] == "\r") l = l.substring(0, l.length - 1);
		b.s = l;
		return l.length;
	}
	close() {}
};

const script = process.argv[2];
global.arguments = process.argv.slice(3);
let src = fs.readFileSync(script, "utf8");
src = src.replace(/^#!.*\n/, "\n");
src = src.replace(/#([A-Za-z_$][\w$]*)\s*\(/g, "_pv_$1(").replace(/this\.#/g, "this._pv_");
try {
	vm.runInThisContext(src, { filename: script });
} catch (e) {
	flush();
	process.stderr.write(String(e && e.message ? e.message : e).split("\n")[0] + "\n");
	process.exit(1);
}
flush();
